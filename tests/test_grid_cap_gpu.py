"""Batches past the grid cap.  grid_for() caps a grid at 2^22 workgroups: the data-pass kernels are then launched
in slices (FEC_LAUNCH_GROUPS, q0 > 0; grp_index swizzles over each slice's own gridDim.x), and the kernels that
launch one workgroup per block or per span (the wave plans k_rlc_plan and k_rlc_plan_wreg, k_rlc_plan_span, the
window encode) switch to a grid-stride loop.  Every test here runs 2^22 + 37 blocks of the smallest symbols with
knob `group` at 1 (one block per group: two slices, the second of 37 workgroups) and knob `interleave` at its
default and at 3.

What this size does not reach: the reg, lane and tile plan kernels take 64, 64 and 16 blocks per workgroup, so
their grid-stride loops start only past 64 * 2^22 (16 * 2^22) blocks; the packed XOR kernels cap their grid at
2^20 workgroups of 256 column pieces, i.e. 2^28 pieces, more than 1 GiB of repairs.  Both run here once round
their loops, as large batches.  The XOR and copy kernels on rows cap at 65536 workgroups and do stride here.

Every status, every recovered mask and every recovered row of the whole batch is compared (numpy, whole
arrays); the CPU oracle's batch calls are fast enough at these sizes to give the expectation for all blocks, and
its per-block calls are run on SAMPLE (the blocks around the cap, the last ones, 40 random ones) besides.
Each test allocates well under 1 GiB, except the span decode: its plan workspace alone
(fecgpu_rlc_decode_workspace(2^22 + 37, 16, 6)) is 896 MiB."""
import numpy as np
import pytest

from oracle_py import DEC_NOTHING, DEC_RECOVERED, DEC_REF_UB, Oracle
from span_model import SpanModel
from test_rows_len_gpu import to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
CAP = 1 << 22
NB = CAP + 37
SAMPLE = [0, 1, CAP - 1, CAP, CAP + 1, NB - 2, NB - 1] + np.random.default_rng(4).choice(NB, 40, replace=False).tolist()
B = np.arange(NB, dtype=np.int64)
MISSING, GUARD, SENT = 0xA5, 0xC3, 0xD7
ILV = [1, 3]


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    e = Engine(0)
    assert e.get_knob("interleave") == 1
    return e


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def model():
    return SpanModel()


class knobs:
    """Several knobs for the duration of a block."""

    def __init__(self, eng, **kv):
        self.eng, self.kv = eng, kv

    def __enter__(self):
        self.old = {k: self.eng.get_knob(k) for k in self.kv}
        for k, v in self.kv.items():
            self.eng.set_knob(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.eng.set_knob(k, v)


def verdict():
    return (torch.full((NB,), 0xEE, dtype=torch.uint8, device=DEV), torch.full((NB, 2), -1, dtype=torch.int64, device=DEV))


def host(st, rec):
    return st.cpu().numpy(), rec.cpu().numpy().view(np.uint64)


def mask_words(lo):
    m = np.zeros((NB, 2), np.uint64)
    m[:, 0] = lo
    return m


def done():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ RLC, packed
class RlcBatch:
    """k3 r2 L4.  fbn_base puts the 24-bit wrap of the block number at block 2^22 + 10, inside the second slice.
    Block b loses source b % 3; in every seventh block both repairs are absent."""
    k, r, L = 3, 2, 4

    def __init__(self, oracle):
        self.base = (1 << 24) - (CAP + 10)
        self.src = np.random.default_rng(1).integers(1, 256, (NB, 3, 4), dtype=np.uint8)
        self.rep = oracle.rlc_encode_batch(self.src, 2, self.base)
        self.miss = B % 3
        self.sp = mask_words((7 & ~(1 << self.miss)).astype(np.uint64))
        self.rp = mask_words(np.where(B % 7 == 0, 0, 3).astype(np.uint64))
        self.work = self.src.copy()
        self.work[B, self.miss] = MISSING
        # the vectorised expectation: one unknown under a non-zero coefficient is always solved
        self.st = np.where(B % 7 == 0, DEC_NOTHING, DEC_RECOVERED).astype(np.uint8)
        self.ok = self.st == DEC_RECOVERED
        self.rec = mask_words(np.where(self.ok, 1 << self.miss, 0).astype(np.uint64))
        ref = self.work.copy()
        st_o, rec_o = oracle.rlc_decode_batch(ref, self.rep, self.sp, self.rp, self.base)
        assert np.array_equal(st_o, self.st) and np.array_equal(rec_o, self.rec)
        assert np.array_equal(ref[self.ok], self.src[self.ok])
        for b in SAMPLE:  # and block by block on the sample, with the block's own number
            fbn = (self.base + b) & 0xFFFFFF
            assert np.array_equal(self.rep[b], oracle.rlc_encode_batch(self.src[b:b + 1], 2, fbn)[0]), b
            one = self.work[b:b + 1].copy()
            st1, rec1 = oracle.rlc_decode_batch(one, self.rep[b:b + 1], self.sp[b:b + 1], self.rp[b:b + 1], fbn)
            assert st1[0] == self.st[b] and np.array_equal(rec1[0], self.rec[b]), b
        assert (self.base + CAP + 10) & 0xFFFFFF == 0


@pytest.fixture(scope="module")
def rlc(oracle):
    return RlcBatch(oracle)


@pytest.mark.parametrize("ilv", ILV)
def test_rlc_encode(eng, oracle, rlc, ilv):
    src = to_dev(rlc.src)
    rep = torch.full((NB, 2, 4), SENT, dtype=torch.uint8, device=DEV)
    with knobs(eng, group=1, interleave=ilv):
        eng.rlc_encode(src, rep, 3, 2, 4, fbn_base=rlc.base)
        torch.cuda.synchronize()
    got = rep.cpu().numpy()
    for b in SAMPLE:
        assert np.array_equal(got[b], rlc.rep[b]), b
    bad = np.flatnonzero((got != rlc.rep).any(axis=(1, 2)))
    assert bad.size == 0, bad[:8]
    del src, rep
    done()


@pytest.mark.parametrize("plan", [0, 1, 2, 3, 4, 5])
def test_rlc_decode_plan_and_apply(eng, rlc, plan):
    """decode_plan + decode_apply in place and decode_apply_packed (interleave 1 and 3 each) under every plan
    kernel.  Plans 1 (k_rlc_plan) and 5 (k_rlc_plan_wreg) launch a workgroup per block, so their grid is capped
    and blocks 2^22 .. 2^22 + 36 are planned on the second turn of their grid-stride loops.  Plans 0 and 3 (reg),
    2 (lane) and 4 (tile) launch 65537 or 262147 workgroups and go round their loops once: those runs cover the
    sliced data pass behind each plan's record format, not the plan kernels' strides."""
    rep, sp, rp = to_dev(rlc.rep), to_dev(rlc.sp), to_dev(rlc.rp)
    ws = eng.alloc_workspace(NB, 3, 2)
    for ilv, packed in ((1, False), (3, False), (1, True), (3, True)):
        work = to_dev(rlc.work)
        st, rec = verdict()
        ws.fill_(SENT)
        dst = torch.full((NB, 2, 4), SENT, dtype=torch.uint8, device=DEV) if packed else None
        with knobs(eng, group=1, interleave=ilv, plan=plan):
            eng.rlc_decode_plan(sp, rp, 3, 2, NB, ws, fbn_base=rlc.base)
            if packed:
                eng.rlc_decode_apply_packed(work, rep, dst, st, rec, 3, 2, 4, NB, ws)
            else:
                eng.rlc_decode_apply(work, rep, st, rec, 3, 2, 4, NB, ws)
            torch.cuda.synchronize()
        st_h, rec_h = host(st, rec)
        tag = (plan, ilv, packed)
        assert np.array_equal(st_h, rlc.st), (tag, np.flatnonzero(st_h != rlc.st)[:8])
        assert np.array_equal(rec_h, rlc.rec), (tag, np.flatnonzero((rec_h != rlc.rec).any(1))[:8])
        got = work.cpu().numpy()
        if packed:
            assert np.array_equal(got, rlc.work), (tag, "src is only read")
            d = dst.cpu().numpy()
            want = np.full((NB, 2, 4), SENT, np.uint8)
            want[rlc.ok, 0] = rlc.src[B, rlc.miss][rlc.ok]  # row 0: the one missing source
            bad = np.flatnonzero((d != want).any(axis=(1, 2)))
        else:
            want = np.where(rlc.ok[:, None, None], rlc.src, rlc.work)
            bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert bad.size == 0, (tag, bad[:8])
        del work, st, rec, dst
    del rep, sp, rp, ws
    done()


# ------------------------------------------------------------------------------------------------ RLC rows, one pass
@pytest.mark.parametrize("ilv", ILV)
def test_rlc_decode_rows_fused(eng, oracle, ilv):
    """k2 r1 L8, every row in one pool (8 bytes of room and 4 guard bytes each), block lengths 5 .. 8.  Block b
    loses source b % 2; every seventh block has no repair (address 0)."""
    k, r, L, stride = 2, 1, 8, 12
    rng = np.random.default_rng(2)
    blk = (5 + B % 4).astype(np.uint32)
    src = rng.integers(1, 256, (NB, k, L), dtype=np.uint8)
    src[np.broadcast_to(np.arange(L)[None, None, :] >= blk[:, None, None], src.shape)] = 0
    rep = oracle.rlc_encode_batch(src, r, 0)  # block numbers 0 .. NB - 1 (< 2^24)
    seeds = (B << 8).astype(np.uint32)
    miss, have_rep = B % 2, B % 7 != 0
    pool = np.full((3 * NB, stride), GUARD, np.uint8)
    live = np.arange(stride)[None, :] < np.repeat(blk, k)[:, None]
    rows = np.full((NB * k, stride), GUARD, np.uint8)
    rows[:, :L] = src.reshape(NB * k, L)
    rows[B * k + miss, :L] = MISSING
    pool[:NB * k] = np.where(live, rows, np.uint8(GUARD))
    reps = np.full((NB, stride), GUARD, np.uint8)
    reps[:, :L] = rep[:, 0]
    pool[NB * k:] = np.where(np.arange(stride)[None, :] < blk[:, None], reps, np.uint8(GUARD))
    want = pool.copy()
    x = (B * k + miss)[have_rep]
    rows[:, :L] = src.reshape(NB * k, L)
    want[x] = np.where(live[x], rows[x], np.uint8(GUARD))
    st_want = np.where(have_rep, DEC_RECOVERED, DEC_NOTHING).astype(np.uint8)
    rec_want = mask_words(np.where(have_rep, 1 << miss, 0).astype(np.uint64))
    for b in SAMPLE:
        srcs = [None if j == miss[b] else src[b, j, :blk[b]] for j in range(k)]
        st1, got1 = oracle.rlc_decode_block(0, srcs, [rep[b, 0, :blk[b]] if have_rep[b] else None], seeds[b:b + 1])
        assert st1 == st_want[b] and sorted(got1) == ([int(miss[b])] if have_rep[b] else []), b
        for v in got1.values():
            assert np.array_equal(v, src[b, miss[b], :blk[b]]), b
    d_pool = to_dev(pool.reshape(-1))
    base = d_pool.data_ptr()
    src_rows = to_dev((base + np.arange(NB * k, dtype=np.int64) * stride).astype(np.uint64))
    rep_rows = to_dev(np.where(have_rep, base + (NB * k + B) * stride, 0).astype(np.uint64))
    src_len = np.repeat(blk, k)
    src_len[B * k + miss] = 0
    t = [to_dev(a) for a in (src_len, blk, blk, seeds, mask_words((3 & ~(1 << miss)).astype(np.uint64)),
                             mask_words(have_rep.astype(np.uint64)))]
    st, rec = verdict()
    ws = eng.alloc_workspace(NB, k, r)
    with knobs(eng, group=1, interleave=ilv):
        eng.rlc_decode_rows_fused(src_rows, t[0], rep_rows, t[1], t[2], t[3], t[4], t[5], st, rec, NB, k, r, L, workspace=ws)
        torch.cuda.synchronize()
    st_h, rec_h = host(st, rec)
    assert np.array_equal(st_h, st_want), np.flatnonzero(st_h != st_want)[:8]
    assert np.array_equal(rec_h, rec_want), np.flatnonzero((rec_h != rec_want).any(1))[:8]
    got = d_pool.cpu().numpy().reshape(3 * NB, stride)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, bad[:8]
    del d_pool, src_rows, rep_rows, t, st, rec, ws
    done()


# ------------------------------------------------------------------------------------------------ XOR
def _xor_turns():
    """By turns: source 0 lost, source 1 lost, a source lost and no repair (NOTHING), nothing lost and no repair
    (REF_UB), nothing lost (NOTHING)."""
    turn = B % 5
    miss = np.where(turn == 0, 0, np.where(turn == 1, 1, np.where(turn == 2, (B >> 1) % 2, -1)))
    have_rep = (turn != 2) & (turn != 3)
    st = np.select([turn < 2, turn == 3], [DEC_RECOVERED, DEC_REF_UB], DEC_NOTHING).astype(np.uint8)
    return miss, have_rep, st


def test_xor_packed(eng, oracle):
    """xor_encode and xor_decode, k2 L4: one thread per column piece.  All rows against numpy XOR, statuses and
    masks against the oracle's batch call.  A large-batch check only: 2^22 + 37 pieces are 16385 workgroups, far
    below these kernels' cap of 2^20, so neither their grid-stride loop nor a second sub-batch runs (that takes
    more than 2^28 pieces).  Of the XOR forms only the rows forms stride at this size (test_xor_rows: 65536
    workgroups of 8 blocks, 8 turns)."""
    k, L = 2, 4
    src = np.random.default_rng(3).integers(1, 256, (NB, k, L), dtype=np.uint8)
    rep_want = (src[:, 0] ^ src[:, 1])[:, None, :]
    for b in SAMPLE:
        assert np.array_equal(oracle.xor_encode_batch(src[b:b + 1])[0], rep_want[b]), b
    d_src = to_dev(src)
    rep = torch.full((NB, 1, L), SENT, dtype=torch.uint8, device=DEV)
    eng.xor_encode(d_src, rep, k, L)
    torch.cuda.synchronize()
    got = rep.cpu().numpy()
    bad = np.flatnonzero((got != rep_want).any(axis=(1, 2)))
    assert bad.size == 0, bad[:8]
    miss, have_rep, st_want = _xor_turns()
    lost = miss >= 0
    sp = mask_words(np.where(lost, 3 & ~(1 << np.maximum(miss, 0)), 3).astype(np.uint64))
    rp = mask_words(have_rep.astype(np.uint64))
    work = src.copy()
    work[B[lost], miss[lost]] = MISSING
    rep_in = np.where(have_rep[:, None, None], rep_want, np.uint8(0x5C))
    ok = st_want == DEC_RECOVERED
    rec_want = mask_words(np.where(ok, 1 << np.maximum(miss, 0), 0).astype(np.uint64))
    ref = work.copy()
    st_o, rec_o = oracle.xor_decode_batch(ref, rep_want, sp, rp)
    assert np.array_equal(st_o, st_want) and np.array_equal(rec_o, rec_want) and np.array_equal(ref[ok], src[ok])
    d_work = to_dev(work)
    st, rec = verdict()
    eng.xor_decode(d_work, to_dev(rep_in), to_dev(sp), to_dev(rp), st, rec, k, L)
    torch.cuda.synchronize()
    st_h, rec_h = host(st, rec)
    assert np.array_equal(st_h, st_want), np.flatnonzero(st_h != st_want)[:8]
    assert np.array_equal(rec_h, rec_want)
    want = np.where(ok[:, None, None], src, work)
    bad = np.flatnonzero((d_work.cpu().numpy() != want).any(axis=(1, 2)))
    assert bad.size == 0, bad[:8]
    del d_src, rep, d_work, st, rec
    done()


def test_xor_rows(eng, oracle):
    """xor_encode_rows and xor_decode_rows, k2 L4: rows of 4 bytes of room and 4 guard bytes in one pool, block
    lengths 1 .. 4, the second source shorter than the block."""
    k, L, stride = 2, 4, 8
    rng = np.random.default_rng(5)
    blk = (1 + B % 4).astype(np.uint32)
    slen = np.stack([blk, (B // 4) % (blk + 1)], 1).astype(np.uint32)
    src = rng.integers(1, 256, (NB, k, L), dtype=np.uint8)
    src[np.arange(L)[None, None, :] >= slen[:, :, None]] = 0
    rep = src[:, 0] ^ src[:, 1]
    col = np.arange(stride)[None, :]

    def rows_of(data, lens):  # [n, L] data -> [n, stride] pool rows: lens bytes, then guard bytes
        out = np.full((data.shape[0], stride), GUARD, np.uint8)
        out[:, :L] = data
        return np.where(col < lens[:, None], out, np.uint8(GUARD))
    for b in SAMPLE:
        ret, one = oracle.xor_encode_block([src[b, j, :slen[b, j]] for j in range(k)])
        assert ret == 0 and np.array_equal(one, rep[b, :blk[b]]), b
    pool = np.concatenate([rows_of(src.reshape(NB * k, L), slen.reshape(-1)), np.full((NB, stride), GUARD, np.uint8)])
    want = pool.copy()
    want[NB * k:] = rows_of(rep, blk)
    d_pool = to_dev(pool.reshape(-1))
    base = d_pool.data_ptr()
    src_rows = (base + np.arange(NB * k, dtype=np.int64) * stride).astype(np.uint64)
    rep_rows = (base + (NB * k + B) * stride).astype(np.uint64)
    d_slen, d_blk = to_dev(slen.reshape(-1)), to_dev(blk)
    eng.xor_encode_rows(to_dev(src_rows), d_slen, to_dev(rep_rows), d_blk, NB, k, L)
    torch.cuda.synchronize()
    got = d_pool.cpu().numpy().reshape(-1, stride)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, bad[:8]
    del d_pool
    # decode: the receiver's rows, the missing source's row poisoned for the block's length
    miss, have_rep, st_want = _xor_turns()
    lost = miss >= 0
    ok = st_want == DEC_RECOVERED
    x = (B * k + np.maximum(miss, 0))
    rx_len = slen.reshape(-1).copy()
    rx = rows_of(src.reshape(NB * k, L), rx_len)
    rx[x[lost]] = rows_of(np.full((int(lost.sum()), L), MISSING, np.uint8), blk[lost])
    pool = np.concatenate([rx, np.where(have_rep[:, None], rows_of(rep, blk), np.uint8(GUARD))])
    want = pool.copy()
    want[x[ok]] = rows_of(src.reshape(NB * k, L)[x[ok]], blk[ok])  # blk bytes: the source, then zeros
    for b in SAMPLE:
        recv = [None if j == miss[b] else src[b, j, :slen[b, j]] for j in range(k)]
        st1, got1 = oracle.xor_decode_block(recv, [rep[b, :blk[b]] if have_rep[b] else None])
        assert st1 == st_want[b], b
        for j, v in got1.items():
            assert j == miss[b] and np.array_equal(v, src[b, j, :blk[b]]), b
    sp = mask_words(np.where(lost, 3 & ~(1 << np.maximum(miss, 0)), 3).astype(np.uint64))
    rp = mask_words(have_rep.astype(np.uint64))
    rec_want = mask_words(np.where(ok, 1 << np.maximum(miss, 0), 0).astype(np.uint64))
    d_pool = to_dev(pool.reshape(-1))
    base = d_pool.data_ptr()
    src_rows = (base + np.arange(NB * k, dtype=np.int64) * stride).astype(np.uint64)
    rep_rows = np.where(have_rep, base + (NB * k + B) * stride, 0).astype(np.uint64)
    st, rec = verdict()
    eng.xor_decode_rows(to_dev(src_rows), d_slen, to_dev(rep_rows), d_blk, to_dev(sp), to_dev(rp), st, rec, NB, k, L)
    torch.cuda.synchronize()
    st_h, rec_h = host(st, rec)
    assert np.array_equal(st_h, st_want), np.flatnonzero(st_h != st_want)[:8]
    assert np.array_equal(rec_h, rec_want)
    got = d_pool.cpu().numpy().reshape(-1, stride)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, bad[:8]
    del d_pool, st, rec, d_slen, d_blk
    done()


# ------------------------------------------------------------------------------------------------ span decode
@pytest.mark.parametrize("ilv", ILV)
def test_span_decode(eng, model, ilv):
    """Spans of 16 columns under windows k6 r1 step 2 (six repairs), L4, one loss per span (column b % 16); every
    seventh span has no repair.  The model on 2^22 + 37 spans costs too much on the host, so the determined
    columns are compared with the sources, and statuses and masks with their vectorised expectation, for all
    spans, and statuses and masks with the model on SAMPLE only."""
    K, R, L, k = 16, 6, 4, 6
    done()  # the largest test of the module: nothing cached from the others beside its 1.6 GB
    src = np.random.default_rng(6).integers(1, 256, (NB, K, L), dtype=np.uint8)
    stream = to_dev(src.reshape(NB * K, L))
    rep = torch.empty((NB, R, L), dtype=torch.uint8, device=DEV)
    for w in range(R):  # window w of every span: the spans' columns are one stream, K symbols apart
        out = torch.empty((NB, 1, L), dtype=torch.uint8, device=DEV)
        eng.rlc_window_encode(stream[2 * w:], out, NB, K, k, 1, L)
        rep[:, w] = out[:, 0]
    torch.cuda.synchronize()
    del stream, out
    lost = B % K
    have_rep = B % 7 != 0
    seed = np.zeros((NB, R), np.uint32)
    off = np.tile((2 * np.arange(R)).astype(np.uint8), (NB, 1))
    nss = np.full((NB, R), k, np.uint8)
    sp = mask_words((0xFFFF & ~(1 << lost)).astype(np.uint64))
    rp = mask_words(np.where(have_rep, (1 << R) - 1, 0).astype(np.uint64))
    st_want = np.where(have_rep, 0, 1).astype(np.uint8)  # RECOVERED: every column lies in a window; NOTHING: m == 0
    rec_want = mask_words(np.where(have_rep, 1 << lost, 0).astype(np.uint64))
    idx = np.array(SAMPLE)
    s = model.solve(K, seed[idx], off[idx], nss[idx], sp[idx], rp[idx])
    assert np.array_equal(s.status, st_want[idx]) and np.array_equal(model.recovered(s, src[idx]), rec_want[idx])
    assert np.array_equal(model.encode(s, src[idx])[have_rep[idx]], rep[idx].cpu().numpy()[have_rep[idx]])
    work = src.copy()
    work[B, lost] = MISSING
    d_work = to_dev(work)
    st, rec = verdict()
    ws = eng.alloc_workspace(NB, K, R)
    with knobs(eng, group=1, interleave=ilv):
        eng.rlc_span_decode(d_work, rep, to_dev(seed), to_dev(off), to_dev(nss), to_dev(sp), to_dev(rp), st, rec, K, R, L,
                            nspans=NB, workspace=ws)
        torch.cuda.synchronize()
    st_h, rec_h = host(st, rec)
    assert np.array_equal(st_h[idx], s.status) and np.array_equal(rec_h[idx], model.recovered(s, src[idx]))
    assert np.array_equal(st_h, st_want), np.flatnonzero(st_h != st_want)[:8]
    assert np.array_equal(rec_h, rec_want), np.flatnonzero((rec_h != rec_want).any(1))[:8]
    want = np.where(have_rep[:, None, None], src, work)
    bad = np.flatnonzero((d_work.cpu().numpy() != want).any(axis=(1, 2)))
    assert bad.size == 0, bad[:8]
    del d_work, rep, st, rec, ws
    done()
