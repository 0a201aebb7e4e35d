"""Every kernel and launch shape a knob selects (fecgpu_set_knob), against the CPU oracle.

The knobs are public ABI and the A/B tools drive them, so a wrong byte behind one goes unnoticed until a
timing is trusted.  Every expectation here comes from the oracle (oracle_py.Oracle, span_model.SpanModel),
never from the engine under another knob value; byte work, so every comparison is exact.  Tests are
parametrised by shape and loop over the knob values inside, each value set through eng.knob() so that it is
put back when an assert fires; the module's engine fixture checks on the way out that every knob is at its
default.  tests/test_knob_ledger.py names these tests knob by knob."""
import contextlib

import numpy as np
import pytest

import test_rows_fused_gpu as RF
from oracle_py import DEC_RECOVERED, Oracle, synth_bytes
from span_model import RECOVERED, SpanModel, pack
from span_model import bits as mask_bits
from test_gpu_parity import DEV, _run_decode_batch, masks_from_lists, to_dev
from test_knob_ledger import knob_defaults

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FBN_WRAP = 2 ** 24 - 3  # the 24-bit block numbers wrap inside every batch
FILL = 0x77


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    e = Engine(0)
    defaults = knob_defaults()
    assert {n: e.get_knob(n) for n in defaults} == defaults, "a knob was left changed before this module"
    yield e
    assert {n: e.get_knob(n) for n in defaults} == defaults, "a knob was left changed by this module"


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


_cache = {}


def cached(key, make):
    """A reference is computed once per module and shared; nobody writes to it."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def enc_case(oracle, k, r, L, nb, fbn_base=FBN_WRAP):
    def make():
        src_h = synth_bytes(nb * k * L, 7000 + 31 * k + r).reshape(nb, k, L)
        return src_h, oracle.rlc_encode_batch(src_h, r, fbn_base)
    return cached(("enc", k, r, L, nb, fbn_base), make)


def encode(eng, src, k, r, L, nb, fbn_base=FBN_WRAP):
    """fecgpu_rlc_encode into a pre-filled buffer -> (return code, repairs)"""
    rep = torch.full((nb, r, L), FILL, dtype=torch.uint8, device=DEV)
    rc = eng.lib.fecgpu_rlc_encode(src.data_ptr(), rep.data_ptr(), nb, k, r, L, fbn_base, None, eng._stream(None))
    torch.cuda.synchronize()
    return rc, rep.cpu().numpy()


class DecodeCase:
    """nb blocks with 0 .. emax erased sources each and every repair present: the damaged rows, the masks and
    the oracle's verdict (status, recovered masks, rows after the decode)."""

    def __init__(self, oracle, k, r, L, nb, emax, fbn_base=FBN_WRAP):
        rng = np.random.default_rng([k, r, L, nb])
        self.k, self.r, self.L, self.nb, self.fbn_base = k, r, L, nb, fbn_base
        self.src, self.rep = enc_case(oracle, k, r, L, nb, fbn_base)
        self.missing = [sorted(rng.choice(k, int(rng.integers(0, emax + 1)), replace=False).tolist()) for _ in range(nb)]
        self.sp = masks_from_lists(nb, k, [[j for j in range(k) if j not in m] for m in self.missing])
        self.rp = masks_from_lists(nb, r, [list(range(r))] * nb)
        self.work = self.src.copy()
        for b, m in enumerate(self.missing):
            self.work[b, m] = 0xA5
        self.ref = self.work.copy()
        self.st, self.rec = oracle.rlc_decode_batch(self.ref, self.rep, self.sp, self.rp, fbn_base)
        self.present = mask_bits(self.sp, k)
        self.recd = mask_bits(self.rec, k)
        assert np.array_equal(self.ref[self.recd], self.src[self.recd])  # the oracle's own round trip
        # the reference gives up on a few per cent of the patterns and a block without a loss has nothing to
        # recover: most blocks still exercise the data pass
        assert 2 * int((self.st == DEC_RECOVERED).sum()) >= nb, (k, r, L, nb)

    def check(self, got, st, rec, tag):
        assert np.array_equal(st, self.st), (tag, np.flatnonzero(st != self.st)[:8])
        assert np.array_equal(rec, self.rec), (tag, np.flatnonzero((rec != self.rec).any(1))[:8])
        assert np.array_equal(got[self.recd], self.ref[self.recd]), tag    # recovered rows
        assert np.array_equal(got[self.present], self.src[self.present]), tag  # received rows are never touched
        idle = self.st != DEC_RECOVERED
        assert np.array_equal(got[idle], self.work[idle]), tag             # nor is a block that is not recovered


def dec_case(oracle, k, r, L, nb, emax):
    return cached(("dec", k, r, L, nb, emax), lambda: DecodeCase(oracle, k, r, L, nb, emax))


def decode_in_place(eng, c, tag):
    _, got, st, rec = _run_decode_batch(eng, c.k, c.r, c.L, c.src, c.rep, c.sp, c.rp, fbn_base=c.fbn_base)
    c.check(got, st, rec, tag)


# ------------------------------------------------------------------------------- a. encode tiling
# (k, r, L, nb), the smallest shapes that reach each branch of k_rlc_encode_bs / k_rlc_encode_bs2<16, false>
# under enc_tile_rt x enc_tile_waves:
#  - 16-B pieces with a pulled-back last piece; r a multiple of no rt * W, nb a multiple of no group size;
#    k >= the ring depth, so rt 16 takes the ring body with W waves
#  - 4-B pieces; k below the ring depth: rt 16 stays on the register body
#  - 8-B pieces; r < rt from rt 4 on; at rt 1, W 4 the last wave owns no repair
#  - two column chunks with a ragged last piece; r > 16: rt 16 launches twice; W > 1 on a multi-chunk symbol
#    takes the ring body without chunk waves
#  - the headline shape
TILE_SHAPES = [(5, 7, 20, 67), (3, 5, 4, 130), (6, 3, 8, 65), (33, 17, 2052, 9), (16, 4, 1200, 300)]
TILE_RT, TILE_W = (1, 2, 4, 8, 16), (1, 2, 3, 4)


def encode_under(eng, knobs, src, want, k, r, L, nb):
    """One encode with the knobs {name: value} set: None when it returned FECGPU_OK and the oracle's repairs,
    else what went wrong."""
    with contextlib.ExitStack() as stack:
        for n, v in knobs.items():
            stack.enter_context(eng.knob(n, v))
        rc, got = encode(eng, src, k, r, L, nb)
    if rc != 0:
        return knobs, rc, eng.err(), "no repair written" if (got == FILL).all() else "some repairs written"
    if not np.array_equal(got, want):
        return knobs, "repairs differ at", np.argwhere(got != want)[:4].tolist()
    return None


@pytest.mark.parametrize("k,r,L,nb", TILE_SHAPES)
def test_a_encode_tiling(eng, oracle, k, r, L, nb):
    """Tiles of 1, 2, 4, 8 and 16 repairs with 1 .. 4 waves splitting a group's repairs (the small-batch LDS
    kernel is bypassed whenever enc_tile_rt is set): the oracle's repairs for every pair."""
    src_h, want = enc_case(oracle, k, r, L, nb)
    src = to_dev(src_h)
    for rt in TILE_RT:
        for W in TILE_W:
            assert not encode_under(eng, {"enc_tile_rt": rt, "enc_tile_waves": W}, src, want, k, r, L, nb)


@pytest.mark.parametrize("ilv", [0, 3])
def test_a_encode_tiling_group_order(eng, oracle, ilv):
    """The same grid with contiguous groups (interleave 0) and with the XCD-aware group order (3)."""
    k, r, L, nb = TILE_SHAPES[0]
    src_h, want = enc_case(oracle, k, r, L, nb)
    src = to_dev(src_h)
    for rt in TILE_RT:
        for W in TILE_W:
            assert not encode_under(eng, {"interleave": ilv, "enc_tile_rt": rt, "enc_tile_waves": W}, src, want,
                                    k, r, L, nb)


def test_a_encode_group_cap(eng, oracle):
    """Knob group on an encode: a cap of 1 and of 3 blocks per group (3 halves the 64 / RT default down to 2)
    under the default tiling."""
    k, r, L, nb = TILE_SHAPES[0]
    src_h, want = enc_case(oracle, k, r, L, nb)
    src = to_dev(src_h)
    for cap in (1, 3):
        assert not encode_under(eng, {"group": cap}, src, want, k, r, L, nb)


# ------------------------------------------------------------------------------- b. LDS of the multi-wave encodes
# Tiles of 1 and 2 repairs keep 8 bytes of coefficient row per source and start from groups of 64 and 32
# blocks, so from k = 33 .. 64 on one wave's rows reach bs_group's 32 KiB cap; a workgroup of 3 or 4 waves
# then asks for 96 - 128 KiB of dynamic LDS and nothing raises the kernel's limit first.  On gfx950 the runtime
# takes such a launch as it is (a workgroup may use the CU's 160 KiB), so these shapes work today; the tests
# pin that they keep returning FECGPU_OK with the right bytes, whatever a later runtime or group rule does.
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("k", [48, 64, 128])
def test_b_multi_wave_encode_lds(eng, oracle, k, r):
    """min_groups 0 keeps the per-shape group sizes at 300 blocks.  Every multi-wave launch shape -- adjacent
    groups on 2 or 4 waves, a group's repairs split over 2 .. 4 waves -- returns FECGPU_OK and the oracle's
    repairs."""
    L, nb = 4, 300
    src_h, want = enc_case(oracle, k, r, L, nb)
    src = to_dev(src_h)
    sets = [{"enc_block_waves": bw} for bw in (2, 4)]
    sets += [{"enc_tile_rt": rt, "enc_tile_waves": W} for rt in (1, 2) for W in (2, 3, 4)]
    bad = [encode_under(eng, {"min_groups": 0, **knobs}, src, want, k, r, L, nb) for knobs in sets]
    assert not any(bad), [x for x in bad if x]


def test_b_multi_wave_encode_lds_at_scale(eng, oracle):
    """The route an A/B run takes: no min_groups override, a batch large enough (65 539 blocks, 12.6 MB of
    sources) that the groups stay at 64 blocks, enc_block_waves 4."""
    k, r, L, nb = 48, 1, 4, 65539
    assert (nb + 63) // 64 >= eng.get_knob("min_groups")
    src_h, want = enc_case(oracle, k, r, L, nb)
    assert not encode_under(eng, {"enc_block_waves": 4}, to_dev(src_h), want, k, r, L, nb)


# ------------------------------------------------------------------------------- c. chunk_waves
CHUNK_SHAPES = [(9, 16, 2064, 70), (40, 16, 4100, 70)]  # nb > 64 keeps the small-batch kernels out


@pytest.mark.parametrize("k,r,L,nb", CHUNK_SHAPES)
def test_c_chunk_waves_encode_and_decode(eng, oracle, k, r, L, nb):
    """Symbols of two and three column chunks on the 16-repair / 16-unknown ring bodies: four chunk waves per
    workgroup (1) or one wave coding the chunks in turn (0)."""
    c = dec_case(oracle, k, r, L, nb, min(k, 16))
    src = to_dev(c.src)
    for v in (0, 1):
        with eng.knob("chunk_waves", v):
            rc, got = encode(eng, src, k, r, L, nb)
            assert rc == 0, (v, eng.err())
            assert np.array_equal(got, c.rep), v
            decode_in_place(eng, c, v)


def test_c_chunk_waves_apply_forms(eng, oracle):
    """fecgpu_rlc_decode_apply_packed and _apply_to on the second shape: recovered rows where each form puts
    them, every other byte of dst and all of src untouched."""
    k, r, L, nb = CHUNK_SHAPES[1]
    c = dec_case(oracle, k, r, L, nb, min(k, 16))
    em = min(k, r)
    work, rep = to_dev(c.work), to_dev(c.rep)
    ws = eng.alloc_workspace(nb, k, r)
    eng.rlc_decode_plan(to_dev(c.sp), to_dev(c.rp), k, r, nb, ws, fbn_base=c.fbn_base)
    ok = c.st == DEC_RECOVERED
    for v in (0, 1):
        for packed in (True, False):
            dst = torch.full((nb, em, L) if packed else (nb, k, L), 0xC3, dtype=torch.uint8, device=DEV)
            st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
            rec = torch.full((nb, 2), -1, dtype=torch.int64, device=DEV)
            with eng.knob("chunk_waves", v):
                (eng.rlc_decode_apply_packed if packed else eng.rlc_decode_apply_to)(work, rep, dst, st, rec, k, r, L,
                                                                                     nb, ws)
                torch.cuda.synchronize()
            tag = (v, packed)
            assert np.array_equal(st.cpu().numpy(), c.st), tag
            assert np.array_equal(rec.cpu().numpy().view(np.uint64), c.rec), tag
            assert np.array_equal(work.cpu().numpy(), c.work), tag  # src is only read
            got = dst.cpu().numpy()
            for b in range(nb):
                m = c.missing[b]
                for u, j in enumerate(m):
                    row = got[b, u] if packed else got[b, j]
                    if c.recd[b, j]:
                        assert np.array_equal(row, c.src[b, j]), (tag, b, j)
                    elif not ok[b]:
                        assert (row == 0xC3).all(), (tag, b, j)
                if packed:
                    assert (got[b, len(m):] == 0xC3).all(), (tag, b)
                else:
                    assert (got[b, c.present[b]] == 0xC3).all(), (tag, b)


def test_c_chunk_waves_span_decode(eng):
    """One packed fecgpu_rlc_span_decode case, K 40, R 16 full-width repairs, L 4100: its 16-unknown tiles
    ride the same ring kernel.  Expectation: tests/span_model.py, the repairs from its own coefficient rows."""
    K, R, L, nb = 40, 16, 4100, 12
    model = SpanModel()
    rng = np.random.default_rng(4100)
    src = synth_bytes(nb * K * L, 40).reshape(nb, K, L)
    seed = np.tile(np.arange(R, dtype=np.uint32), (nb, 1))
    off = np.zeros((nb, R), np.uint8)
    nss = np.full((nb, R), K, np.uint8)
    present = np.ones((nb, K), bool)
    for b in range(nb):
        present[b, rng.choice(K, 16 if b % 2 == 0 else int(rng.integers(1, 19)), replace=False)] = False
    rpresent = np.ones((nb, R), bool)
    rpresent[1::4, 0] = False
    sp, rp = pack(present), pack(rpresent)
    rep = model.encode(model.solve(K, seed, off, nss, sp, pack(np.ones((nb, R), bool))), src)
    s = model.solve(K, seed, off, nss, sp, rp)
    assert 2 * int((s.status == RECOVERED).sum()) >= nb and (s.det.sum(1)[::2] == 16).all()
    work = np.where(s.miss[:, :, None], np.uint8(0xA5), src)
    rep_w = np.where(s.selected[:, :, None], rep, np.uint8(0x5A))  # a repair the decode does not select is not read
    want = model.expected_rows(s, work, src)
    for v in (0, 1):
        w, rd = to_dev(work), to_dev(rep_w)
        st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
        rec = torch.full((nb, 2), -1, dtype=torch.int64, device=DEV)
        with eng.knob("chunk_waves", v):
            eng.rlc_span_decode(w, rd, torch.from_numpy(seed.view(np.int32)).to(DEV), to_dev(off), to_dev(nss),
                                to_dev(sp), to_dev(rp), st, rec, K, R, L, nspans=nb)
            torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), s.status), v
        assert np.array_equal(rec.cpu().numpy().view(np.uint64), model.recovered(s, src)), v
        assert np.array_equal(w.cpu().numpy(), want), v
        assert np.array_equal(rd.cpu().numpy(), rep_w), v


# ------------------------------------------------------------------------------- d. dec_waves, plan
DEC_WAVES = (1, 3, 8)  # the workgroup's LDS padded to 40 KiB, 13.3 KiB and 5 KiB


@pytest.mark.parametrize("k,r,L,nb", [(16, 4, 1200, 300), (128, 16, 8, 70)])
def test_d_dec_waves_decode(eng, oracle, k, r, L, nb):
    """The register-prefetch recover kernel under an occupancy cap: the headline shape and the widest block
    on the 16-unknown tile (8-B pieces keep it off the ring)."""
    c = dec_case(oracle, k, r, L, nb, min(k, r))
    for v in DEC_WAVES:
        with eng.knob("dec_waves", v):
            decode_in_place(eng, c, v)


def test_d_dec_waves_rows_fused(eng, oracle):
    """fecgpu_rlc_decode_rows_fused (the row form of the same launch shape) on a ragged pool."""
    c = cached("fused", lambda: RF.FusedDecodeCase(np.random.default_rng([RF.SEED, 16, 4]), oracle, 300, 16, 4, 1200))
    assert 2 * c.n_recovered >= c.nb
    for v in DEC_WAVES:
        with eng.knob("dec_waves", v):
            got, st, rec = RF.run_decode(eng, c)
        RF.check_decode(c, got, st, rec, v)


def test_d_plan_kernels_decode(eng, oracle):
    """Every plan kernel forced in turn (wave, lane, register, tile, wave in registers; k 16, r 4 fits them
    all), then the data pass: the oracle's status, masks and rows."""
    c = dec_case(oracle, 16, 4, 1200, 300, 4)
    for v in (1, 2, 3, 4, 5):
        with eng.knob("plan", v):
            decode_in_place(eng, c, v)


# ------------------------------------------------------------------------------- e. host path
def pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


def window_case(oracle, k, r, L, nw, step):
    def make():
        nrows = (nw - 1) * step + k
        sym = synth_bytes(nrows * L, 515).reshape(nrows, L)
        wrow = (np.arange(nw) * step).astype(np.uint32)
        want = np.stack([np.stack(oracle.rlc_encode_block(0, list(sym[w:w + k]), r)[1]) for w in wrow])
        return sym, wrow, want
    return cached(("win", k, r, L, nw, step), make)


def test_e_zc_read_0_stages_page_locked_buffers(eng, oracle):
    """Knob zc_read 0 on page-locked buffers: the three call sites of host_path.hip stage by copies --
    fecgpu_rlc_encode_host, fecgpu_rlc_decode_host and fecgpu_rlc_window_encode_host (the last with both
    values of window_sc) -- in sub-batches over three streams."""
    from pquic_amd import HostPath
    k, r, L, nb = 16, 4, 1200, 200
    c = dec_case(oracle, k, r, L, nb, 4)
    sym, wrow, wwant = window_case(oracle, k, r, L, 50, 8)
    hp = HostPath(0, 3, 1 << 20)
    try:
        with eng.knob("zc_read", 0):
            srcp, repp = pinned(c.src), pinned(np.full((nb, r, L), FILL, np.uint8))
            hp.rlc_encode(srcp, repp, nb, k, r, L, c.fbn_base)
            assert np.array_equal(repp.numpy(), c.rep)
            assert np.array_equal(srcp.numpy(), c.src)

            workp, repp = pinned(c.work), pinned(c.rep)
            spp, rpp = pinned(c.sp.view(np.int64)), pinned(c.rp.view(np.int64))
            st, rec = pinned(np.full(nb, 0xEE, np.uint8)), pinned(np.full((nb, 2), -1, np.int64))
            hp.rlc_decode(workp, repp, spp, rpp, st, rec, nb, k, r, L, c.fbn_base)
            c.check(workp.numpy(), st.numpy(), rec.numpy().view(np.uint64), "host decode")
            assert np.array_equal(repp.numpy(), c.rep)

            symp = pinned(sym)
            for sc in (1, 0):
                wrep = pinned(np.full(wwant.shape, FILL, np.uint8))
                with eng.knob("window_sc", sc):
                    hp.rlc_window_encode(symp, len(sym), wrow, wrep, len(wrow), k, r, L)
                assert np.array_equal(wrep.numpy(), wwant), sc
    finally:
        hp.close()


@pytest.mark.parametrize("sc", [0, 2])
def test_e_window_encode_kernels(eng, oracle, sc):
    """fecgpu_rlc_window_encode with overlapping windows on the block-at-a-time kernel (window_sc 0, one
    window per group) and on the shared-coefficient kernel wherever it applies (2)."""
    k, r, L, nw, step = 16, 4, 1200, 50, 8
    sym, _, want = window_case(oracle, k, r, L, nw, step)
    rep = torch.full((nw, r, L), FILL, dtype=torch.uint8, device=DEV)
    with eng.knob("window_sc", sc):
        eng.rlc_window_encode(to_dev(sym), rep, nw, step, k, r, L)
        torch.cuda.synchronize()
    assert np.array_equal(rep.cpu().numpy(), want)


@pytest.mark.parametrize("nstreams", [3, 1])
def test_e_pacer_slices(eng, oracle, nstreams):
    """Zero-copy encode cut into slices (yield_always 1; a 1 KiB slice is the Pacer's floor of 32 blocks):
    at most yield_depth slices in flight, over yield_streams of the context's streams -- more than a context
    of one or three streams has, so the clamp runs -- and with a gate that no pending hook ever closes.
    Every call gives the oracle's repairs in exactly ceil(200 / 32) slices and waits for no hook."""
    from pquic_amd import HostPath
    k, r, L, nb = 16, 4, 1200, 200
    src_h, want = enc_case(oracle, k, r, L, nb)
    slices = -(-nb // 32)
    hp = HostPath(0, nstreams, 64 << 20)
    try:
        srcp = pinned(src_h)
        with eng.knob("yield_always", 1), eng.knob("yield_slice_kb", 1):
            for depth, streams, gate in [(1, 1, 0), (1, 4, 0), (2, 1, 0), (2, 4, 0), (16, 2, 200), (2, 4, 200)]:
                repp = pinned(np.full((nb, r, L), FILL, np.uint8))
                with eng.knob("yield_depth", depth), eng.knob("yield_streams", streams), \
                        eng.knob("yield_gate_us", gate):
                    before = eng.stats()
                    hp.rlc_encode(srcp, repp, nb, k, r, L, FBN_WRAP)
                    after = eng.stats()
                tag = (depth, streams, gate)
                assert np.array_equal(repp.numpy(), want), tag
                assert after["yield_slices"] - before["yield_slices"] == slices, tag
                assert after["yield_waits"] == before["yield_waits"], tag
    finally:
        hp.close()
