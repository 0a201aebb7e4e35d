"""The header's "graph-capturable" promise (include/fecgpu.h): call sequences of the device forms captured into a
HIP graph on one side stream and replayed.

Every sequence runs once eagerly on the stream (first-use initialisation may happen there), is captured on that
one stream -- every engine call inside the capture must return FECGPU_OK -- and is replayed three times.  Before
each replay, device copies on the same stream overwrite payload, masks, seeds and lengths with another case of
the same shape and refill every output, workspace and scratch buffer with the sentinel; each replay is compared
bit for bit with the CPU oracle or the span model.  Graphs are linear: one stream, no forked branches.

The row forms run on a fixed layout (row x at x * (L + 16) in one pool, 16 sentinel bytes behind every row), so
the address tables a graph holds stay valid while lengths and contents change."""
import numpy as np
import pytest

import test_streams_gpu as TS
from oracle_py import DEC_RECOVERED, Oracle
from span_model import SpanModel, pack
from test_streams_gpu import ABSENT, MISSING, PAY, SENT, Case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 16
REPLAYS = 3


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(0)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def model():
    return SpanModel()


def capture_and_replay(make):
    """make(variant) -> Case.  Variant 0 owns the buffers the graph refers to; variants 1 .. 3 are loaded into
    them before a replay and judge its result."""
    cases = [make(v) for v in range(REPLAYS + 1)]
    a = cases[0]
    for c in cases[1:]:
        assert [(x[0].shape, x[0].dtype) for x in c.ins] == [(x[0].shape, x[0].dtype) for x in a.ins]
        assert c.layout() == a.layout(), "the address tables of the shape's cases differ"
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        a.stage(late=False)
        a.run(S)
        S.synchronize()
        a.check(a.fetch())
        a.stage(late=False)
    S.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        a.run(S)  # the engine wrappers raise on any status but FECGPU_OK
    try:
        for c in cases[1:]:
            with torch.cuda.stream(S):
                for t, v in a.outs:
                    t.fill_(v)
                for (live, _, _), (_, real, _) in zip(a.ins, c.ins):
                    live.copy_(real)
                g.replay()
                S.synchronize()
                got = a.fetch()
            c.check(got)
    finally:
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ packed sequences
@pytest.mark.parametrize("k,r,L,nb,e_min", [(16, 4, 1200, 300, 0), (40, 20, 100, 70, 17)])
def test_encode_plan_apply_packed(eng, oracle, k, r, L, nb, e_min):
    """The bench's path: rlc_encode, decode_plan, decode_apply_packed."""
    capture_and_replay(lambda v: TS._encode_then_decode(eng, oracle, TS.Packed.get(oracle, k, r, L, nb, e_min=e_min, variant=v)))


def test_decode_one_launch(eng, oracle):
    capture_and_replay(lambda v: TS.build_decode(eng, oracle, 16, 4, 1200, 7, "decode", variant=v))


def test_decode_full(eng, oracle):
    capture_and_replay(lambda v: TS.build_full(eng, oracle, 16, 8, 256, 100, "decode_full", variant=v))


# ------------------------------------------------------------------------------------------------ fixed-layout rows
class Rows:
    """n rows of room L at a fixed stride in one pool image."""

    def __init__(self, n, L):
        self.n, self.L, self.stride = n, L, L + GUARD
        self.image = np.full(n * self.stride + 64, SENT, np.uint8)

    def off(self, x):
        return 64 + np.asarray(x, np.int64) * self.stride

    def put(self, img, x, data):
        o = int(self.off(x))
        img[o:o + len(data)] = data

    def table(self, base, first, n):
        return (base + self.off(first + np.arange(n))).astype(np.uint64)


def _ragged_batch(rng, nb, k, L, min_len):
    blk = rng.integers(max(min_len, 1), L + 1, nb).astype(np.uint32)
    blk[:3] = [L, 1, L - 1]
    src_len = rng.integers(min_len, blk[:, None] + 1, (nb, k)).astype(np.uint32)
    src_len[np.arange(nb), rng.integers(0, k, nb)] = blk
    src = np.zeros((nb, k, L), np.uint8)
    for b in range(nb):
        for j in range(k):
            src[b, j, :src_len[b, j]] = rng.integers(1, 256, int(src_len[b, j]), dtype=np.uint8)
    return blk, src_len, src


def _erase(rng, nb, k, r):
    present, rpresent = np.ones((nb, k), bool), np.zeros((nb, r), bool)
    for b in range(nb):
        e = int(rng.integers(1, min(k, r) + 1))
        present[b, rng.choice(k, e, replace=False)] = False
        nrep = e - 1 if b % 8 == 7 else int(rng.integers(e, r + 1))
        rpresent[b, rng.choice(r, nrep, replace=False)] = True
    return present, rpresent


def rlc_rows_roundtrip(eng, oracle, k, r, L, nb, variant):
    """encode_rows_fused from the sender's rows into the repair rows, then decode_rows_fused on the receiver's
    rows (missing ones poisoned) and those repairs."""
    rng = np.random.default_rng([k, r, L, nb, variant])
    blk, src_len, src = _ragged_batch(rng, nb, k, L, 1)
    fbn_h = rng.integers(0, 1 << 24, nb).astype(np.uint32)
    seeds_h = ((fbn_h[:, None].astype(np.uint64) << 8) | np.arange(r, dtype=np.uint64)).astype(np.uint32)
    present, rpresent = _erase(rng, nb, k, r)
    R = Rows(2 * nb * k + nb * r, L)  # sender's sources, repairs, receiver's sources
    tx, rp0, rx = 0, nb * k, nb * k + nb * r
    img = R.image.copy()
    reps, verdict, rows = [], [], {}
    for b in range(nb):
        srcs = [src[b, j, :src_len[b, j]] for j in range(k)]
        ret, rep = oracle.rlc_encode_block(int(fbn_h[b]), srcs, r)
        assert ret == 0 and all(len(x) == blk[b] for x in rep)
        reps.append(rep)
        for j in range(k):
            R.put(img, tx + b * k + j, srcs[j])
            R.put(img, rx + b * k + j, srcs[j] if present[b, j] else np.full(blk[b], MISSING, np.uint8))
        st, got = oracle.rlc_decode_block(0, [srcs[j] if present[b, j] else None for j in range(k)],
                                          [rep[i] if rpresent[b, i] else None for i in range(r)], seeds_h[b])
        verdict.append(st)
        for j, v in got.items():
            assert np.array_equal(v, src[b, j, :blk[b]])
            rows[(b, j)] = v
    status = np.array(verdict, np.uint8)
    assert 2 * (status == DEC_RECOVERED).sum() >= nb
    recb = np.zeros((nb, k), bool)
    for b, j in rows:
        recb[b, j] = True
    want = img.copy()
    for b in range(nb):
        for i in range(r):
            R.put(want, rp0 + b * r + i, reps[b][i])
    for (b, j), v in rows.items():
        R.put(want, rx + b * k + j, v)
    free = [(b, j) for b in np.flatnonzero(status == DEC_RECOVERED) for j in np.flatnonzero(~present[b] & ~recb[b])]

    c = Case(eng)
    pool = c.inp(img, PAY)
    base = pool.data_ptr()
    t_tx, t_rep, t_rx = (c.const(R.table(base, f, n)) for f, n in ((tx, nb * k), (rp0, nb * r), (rx, nb * k)))
    slen, blen = c.inp(src_len.reshape(-1), 0), c.inp(blk, 0)
    rlen = c.inp(np.repeat(blk, r), 0)
    fbn, seeds = c.inp(fbn_h, 0), c.inp(seeds_h, 0)
    sp, rp = c.inp(pack(present), -1), c.inp(pack(rpresent), -1)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, k, r))

    def run(s):
        eng.rlc_encode_rows_fused(t_tx, slen, t_rep, blen, nb, k, r, L, fbn=fbn, stream=s)
        eng.rlc_decode_rows_fused(t_rx, slen, t_rep, rlen, blen, seeds, sp, rp, st, rec, nb, k, r, L, workspace=ws, stream=s)
    c.run = run
    c.reads = {"pool": pool, "st": st, "rec": rec}

    def check(g):
        assert np.array_equal(g["st"], status) and np.array_equal(g["rec"], pack(recb))
        w = want.copy()
        for b, j in free:  # a missing source of a RECOVERED block whose bit stays clear: blk bytes of anything
            o = int(R.off(rx + b * k + j))
            w[o:o + blk[b]] = g["pool"][o:o + blk[b]]
        assert np.array_equal(g["pool"], w), np.flatnonzero(g["pool"] != w)[:8]
    c.check = check
    return c


def test_rows_fused_encode_then_decode(eng, oracle):
    capture_and_replay(lambda v: rlc_rows_roundtrip(eng, oracle, 12, 6, 1204, 70, v))


def xor_rows_roundtrip(eng, oracle, k, L, nb, variant):
    """xor_encode_rows from the sender's rows, then xor_decode_rows on the receiver's rows and that repair."""
    rng = np.random.default_rng([k, L, nb, variant, 5])
    _, src_len, src = _ragged_batch(rng, nb, k, L, 1)
    blk = src_len.max(1).astype(np.uint32)
    R = Rows(2 * nb * k + nb, L)
    tx, rp0, rx = 0, nb * k, nb * k + nb
    img = R.image.copy()
    present = np.ones((nb, k), bool)
    rpresent = np.ones((nb, 1), bool)
    status, recb = np.zeros(nb, np.uint8), np.zeros((nb, k), bool)
    outs = []
    for b in range(nb):
        turn = b % 4
        present[b, rng.choice(k, (1, 1, 2, 0)[turn], replace=False)] = False
        rpresent[b, 0] = b % 8 not in (1, 3)  # NOTHING with one source missing, REF_UB with none
        srcs = [src[b, j, :src_len[b, j]] for j in range(k)]
        ret, rep = oracle.xor_encode_block(srcs)
        assert ret == 0 and len(rep) == blk[b]
        outs.append((rp0 + b, rep))
        for j in range(k):
            R.put(img, tx + b * k + j, srcs[j])
            R.put(img, rx + b * k + j, srcs[j] if present[b, j] else np.full(blk[b], MISSING, np.uint8))
        st, got = oracle.xor_decode_block([srcs[j] if present[b, j] else None for j in range(k)],
                                          [rep if rpresent[b, 0] else None])
        status[b] = st
        for j, v in got.items():
            recb[b, j] = True
            outs.append((rx + b * k + j, v))
    assert (status == DEC_RECOVERED).sum() >= nb // 4 and len(set(status.tolist())) == 3
    want = img.copy()
    for x, v in outs:
        R.put(want, x, v)
    c = Case(eng)
    pool = c.inp(img, PAY)
    base = pool.data_ptr()
    t_tx, t_rep, t_rx = (c.const(R.table(base, f, n)) for f, n in ((tx, nb * k), (rp0, nb), (rx, nb * k)))
    slen, blen = c.inp(src_len.reshape(-1), 0), c.inp(blk, 0)
    sp, rp = c.inp(pack(present), -1), c.inp(pack(rpresent), -1)
    st, rec = c.verdict(nb)

    def run(s):
        eng.xor_encode_rows(t_tx, slen, t_rep, blen, nb, k, L, stream=s)
        eng.xor_decode_rows(t_rx, slen, t_rep, blen, sp, rp, st, rec, nb, k, L, stream=s)
    c.run = run
    c.reads = {"pool": pool, "st": st, "rec": rec}

    def check(g):
        assert np.array_equal(g["st"], status) and np.array_equal(g["rec"], pack(recb))
        assert np.array_equal(g["pool"], want), np.flatnonzero(g["pool"] != want)[:8]
    c.check = check
    return c


def test_xor_rows_encode_then_decode(eng, oracle):
    capture_and_replay(lambda v: xor_rows_roundtrip(eng, oracle, 4, 1200, 300, v))


def window_rows(eng, oracle, k, r, step, L, nw, variant):
    rng = np.random.default_rng([k, r, step, L, nw, variant])
    nrows = (nw - 1) * step + k
    lens = rng.integers(0, L + 1, nrows)
    lens[rng.integers(0, nrows, 5)] = L
    lens[rng.integers(0, nrows, 3)] = 0
    wrow_h = (np.arange(nw) * step).astype(np.uint32)
    blk = np.array([lens[w * step:w * step + k].max() if w % 3 == 0 else int(rng.integers(1, L + 1)) for w in range(nw)],
                   np.uint32)
    R = Rows(nrows + nw * r, L)
    img = R.image.copy()
    data = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in lens]
    for x in range(nrows):
        R.put(img, x, data[x])
    want = img.copy()
    for w in range(nw):
        bl = int(blk[w])
        if not bl:
            continue
        srcs = [data[x][:bl] for x in range(w * step, w * step + k)]
        if max(len(s) for s in srcs) < bl:  # zero-padding to the window's length changes no repair byte
            srcs[0] = np.concatenate([srcs[0], np.zeros(bl - len(srcs[0]), np.uint8)])
        ret, reps = oracle.rlc_encode_block(0, srcs, r)
        assert ret == 0 and all(len(x) == bl for x in reps)
        for i in range(r):
            R.put(want, nrows + w * r + i, reps[i])
    c = Case(eng)
    pool = c.inp(img, PAY)
    base = pool.data_ptr()
    rows, rep_rows = c.const(R.table(base, 0, nrows)), c.const(R.table(base, nrows, nw * r))
    row_len, wrow, blen = c.inp(lens.astype(np.uint32), 0), c.inp(wrow_h, 0), c.inp(blk, 0)
    ws = c.workspace(eng.window_rows_workspace_bytes(nrows, L))
    c.run = lambda s: eng.rlc_window_encode_rows(rows, row_len, nrows, wrow, rep_rows, blen, nw, k, r, L, workspace=ws,
                                                 stream=s)
    c.reads = {"pool": pool}
    c.check = lambda g: np.testing.assert_array_equal(g["pool"], want)
    return c


def test_window_encode_rows(eng, oracle):
    capture_and_replay(lambda v: window_rows(eng, oracle, 30, 5, 10, 1200, 40, v))


def span_rows(eng, model, variant):
    """fecgpu_rlc_span_decode_rows_fused on the multi-tile layout (17 to 21 losses per span), ragged rows."""
    fx, present, rpresent, rep_h, (blk, src_len, rep_len) = TS.span_set(eng, "multi", ragged=True, variant=variant)
    nb, K, R_, L = fx.nb, fx.K, fx.R, fx.L
    sp_h, rp_h = pack(present), pack(rpresent)
    s = model.solve(K, fx.seed, fx.off, fx.nss, sp_h, rp_h)
    assert (s.det.sum(1) > 16).sum() >= 5
    R = Rows(nb * K + nb * R_, L)
    img = R.image.copy()
    for b in range(nb):
        for j in range(K):
            R.put(img, b * K + j, np.full(blk[b], MISSING, np.uint8) if s.miss[b, j] else fx.src[b, j, :src_len[b, j]])
        for i in range(R_):  # a repair the plan does not select is never read: its row is poisoned
            R.put(img, nb * K + b * R_ + i, rep_h[b, i, :rep_len[b, i]] if s.selected[b, i] else np.full(L, ABSENT, np.uint8))
    want = img.copy()
    for b, j in zip(*np.nonzero(s.det)):
        R.put(want, b * K + j, fx.src[b, j, :blk[b]])
    exp_rec = model.recovered(s, fx.src)
    c = Case(eng)
    pool = c.inp(img, PAY)
    base = pool.data_ptr()
    srow, rrow = c.const(R.table(base, 0, nb * K)), c.const(R.table(base, nb * K, nb * R_))
    slen = c.inp(np.where(s.miss, 0, src_len).astype(np.uint32).reshape(-1), 0)
    rlen = c.inp(np.where(s.selected, rep_len, L).astype(np.uint32).reshape(-1), 0)
    blen = c.inp(blk.astype(np.uint32), 0)
    seed, off, nss = c.inp(fx.seed, 0), c.inp(fx.off, 0), c.inp(fx.nss, 0)
    sp, rp = c.inp(sp_h, -1), c.inp(rp_h, -1)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, K, R_))
    c.run = lambda t: eng.rlc_span_decode_rows_fused(srow, slen, rrow, rlen, blen, seed, off, nss, sp, rp, st, rec, nb, K,
                                                     R_, L, workspace=ws, stream=t)
    c.reads = {"st": st, "rec": rec, "pool": pool}

    def check(g):
        assert np.array_equal(g["st"], s.status) and np.array_equal(g["rec"], exp_rec)
        assert np.array_equal(g["pool"], want), np.flatnonzero(g["pool"] != want)[:8]
    c.check = check
    return c


def test_span_decode_rows_fused(eng, model):
    capture_and_replay(lambda v: span_rows(eng, model, v))
