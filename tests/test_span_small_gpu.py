"""Span decode of a few spans in one launch (k_rlc_span_decode_small behind fecgpu_rlc_span_decode_rows_fused)
against the numpy model (span_model.py), byte for byte: status, recovered[], every row of a byte pool that
holds the ragged rows with sentinels between them -- determined rows hold the original, missing rows and the
row of every repair the decode must not read are poisoned and stay so, no repair is written.  The loss patterns
are fixed; the asserts on the model's solution say what each is for."""
import contextlib

import numpy as np
import pytest

from span_model import NOTHING, RECOVERED, SINGULAR, pack
from test_span_decode_gpu import Pool, Spans, eng, host_out, model, new_out, to_dev  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENGTHS = [4, 36, 64, 1200]
FIVE = [(5 * o, 30, 1) for o in range(5)]  # K 50: five windows (o, 30, 1), o = 0, 5, ..., 20


@contextlib.contextmanager
def knob(eng, name, value):
    old = eng.get_knob(name)
    eng.set_knob(name, value)
    try:
        yield
    finally:
        eng.set_knob(name, old)


class Batch:
    """nb spans of one shape with a loss pattern each: patterns[b] = (lost columns, lost repairs); ragged lengths
    (every source cut to a length of its own, a repair as long as the longest source of its window, blk_len
    the longest repair received or, without one, the longest source), the rows in a Pool."""

    def __init__(self, eng, model, K, windows, L, patterns, seed, zero=()):
        nb = len(patterns)
        self.fx = fx = Spans(K, L, nb, windows, data_seed=seed)
        rng = np.random.default_rng([seed, L])
        self.src_len = rng.integers(0, L + 1, (nb, K))
        self.src_len[np.arange(nb), rng.integers(0, K, nb)] = L  # one source of every span is L bytes long
        for b, j in zero:  # a source that is all zero although it has a length
            fx.src[b, j] = 0
        fx.src[np.arange(L)[None, None, :] >= self.src_len[:, :, None]] = 0
        self.rep_len = np.stack([self.src_len[:, o:o + n].max(1) for o, n, r in windows for _ in range(r)], 1)
        self.present = np.ones((nb, K), bool)
        self.rpresent = np.ones((nb, fx.R), bool)
        for b, (cols, reps) in enumerate(patterns):
            self.present[b, list(cols)] = False
            self.rpresent[b, list(reps)] = False
        self.sp, self.rp = pack(self.present), pack(self.rpresent)
        self.s = s = model.solve(K, fx.seed, fx.off, fx.nss, self.sp, self.rp)
        got = np.where(self.rpresent, self.rep_len, 0).max(1)
        self.blk = np.where(got > 0, got, self.src_len.max(1)).astype(np.int64)
        assert (self.blk >= 1).all() and (self.src_len <= L).all()
        # a determined source is at most as long as a repair that covers it, so blk_len bytes hold it whole
        assert (np.where(s.det, self.src_len, 0).max(1) <= self.blk).all()
        self.rep = fx.encode(eng)
        self.pool = Pool(fx, s, self.blk, np.minimum(self.src_len, self.blk[:, None]), self.rep_len, self.rep, seed)
        self.slen = np.where(s.miss, 0, self.src_len).astype(np.uint32).reshape(-1)
        self.rlen = np.where(s.selected, self.rep_len, L).astype(np.uint32).reshape(-1)
        self.want_rec = model.recovered(s, fx.src)

    def run(self, eng, stream=None):
        """one fecgpu_rlc_span_decode_rows_fused call on a fresh pool -> (status, recovered, pool bytes)"""
        fx = self.fx
        pool = to_dev(self.pool.bytes)
        srow, rrow = self.pool.tables(pool.data_ptr())
        out = new_out(fx.nb)
        args = [to_dev(a) for a in (srow, self.slen, rrow, self.rlen, self.blk.astype(np.uint32), fx.seed, fx.off,
                                    fx.nss, self.sp, self.rp)]
        torch.cuda.synchronize()
        eng.rlc_span_decode_rows_fused(*args, *out, fx.nb, fx.K, fx.R, fx.L, stream=stream)
        torch.cuda.synchronize()
        st, rec = host_out(out)
        return st, rec, pool.cpu().numpy()

    def check(self, got, what=""):
        st, rec, pool = got
        assert np.array_equal(st, self.s.status), (what, st.tolist(), self.s.status.tolist())
        assert np.array_equal(rec, self.want_rec), (what, np.nonzero((rec != self.want_rec).any(1))[0][:10])
        bad = np.flatnonzero(pool != self.pool.want)
        assert bad.size == 0, (what, bad[:8])


def one_launch(eng, batch, expect=1, what=""):
    """runs the batch, checks it, and asserts by how much the one-launch counter moved"""
    before = eng.span_one_launch_calls()
    got = batch.run(eng)
    assert eng.span_one_launch_calls() - before == expect, what
    batch.check(got, what)
    return got


# the patterns of the K 50 shape: (lost columns, lost repairs)
A, B, C_, D, E = ([22, 23], []), ([22, 23, 48, 49], []), ([0, 1], []), ([], []), ([3], [0, 1, 2, 3, 4])


def five_windows(eng, model, L, patterns, seed=50):
    return Batch(eng, model, 50, FIVE, L, patterns, seed)


@pytest.mark.parametrize("L", LENGTHS)
def test_five_windows_batches_of_1_3_64_and_65(eng, model, L):
    """(a) two losses every window shares: determined jointly, by no window alone; (b) with two more under one
    repair: exactly {22, 23}; (c) two losses under one repair: SINGULAR; (d) no loss, (e) no repair: NOTHING."""
    mix = [A, B, C_, D, E]
    b64 = five_windows(eng, model, L, [mix[b % 5] for b in range(64)])
    s = b64.s
    assert s.status[:5].tolist() == [RECOVERED, RECOVERED, SINGULAR, NOTHING, NOTHING]
    assert np.nonzero(s.det[0])[0].tolist() == [22, 23] and np.nonzero(s.det[1])[0].tolist() == [22, 23]
    assert not model.windows_alone(s, b64.fx.off, b64.fx.nss, propagate=True)[0].any()
    assert not s.det[2:5].any()
    one_launch(eng, b64, 1, "64 spans")
    one_launch(eng, five_windows(eng, model, L, [A], 51), 1, "1 span")
    one_launch(eng, five_windows(eng, model, L, [B, C_, A], 52), 1, "3 spans")
    for p in (C_, D, E):  # a span that decodes nothing, alone in its call: status, zero recovered[], no row touched
        one_launch(eng, five_windows(eng, model, L, [p], 53), 1, "nothing determined")
    one_launch(eng, five_windows(eng, model, L, [mix[b % 5] for b in range(65)], 54), 0, "65 spans: separate launches")


def tile_patterns():
    """K 64 under one window (0, 64, 12): losses at columns 3, 6, ...; 8, 9 and 10 of them"""
    return [(list(range(3, 3 * n + 1, 3)), []) for n in (8, 9, 10, 10)]


@pytest.mark.parametrize("L", LENGTHS)
def test_tile_boundary_loop_and_finalize(eng, model, L):
    """(f) e = 8 fills the tile of 8 unknowns, e = 9 and 10 take the loop in the kernel and its finalize; (g)
    e = 10 with a determined source that is all zero: written as zeros, its recovered bit clear."""
    pats = tile_patterns()
    bt = Batch(eng, model, 64, [(0, 64, 12)], L, pats, 64, zero=[(3, 9)])
    assert bt.s.det.sum(1).tolist() == [8, 9, 10, 10] and (bt.s.status == RECOVERED).all()
    assert bt.s.det[3, 9] and not bt.fx.src[3, 9].any()
    assert not (int(bt.want_rec[3, 0]) >> 9) & 1 and (int(bt.want_rec[3, 0]) >> 12) & 1 == int(bt.fx.src[3, 12].any())
    one_launch(eng, bt, 1, "e = 8, 9, 10, 10")
    for i, p in enumerate(pats):
        one_launch(eng, Batch(eng, model, 64, [(0, 64, 12)], L, [p], 65 + i, zero=[(0, 9)] if i == 3 else ()), 1, i)


@pytest.mark.parametrize("L", LENGTHS)
def test_large_shapes(eng, model, L):
    """(h) K 128, R 32, banded, 12 determined in two tiles, the largest shape of the LDS rule's static_assert;
    (i) K 125, R 20: five determined, none by a window alone; (j) K 30, R 6, seven losses: SINGULAR; (k) K 1."""
    h = Batch(eng, model, 128, [(3 * o, 30, 1) for o in range(32)], L, [(list(range(50, 62)), [])] * 3, 128)
    assert h.fx.R == 32 and (h.s.det.sum(1) == 12).all() and (h.s.det == h.s.miss).all()
    one_launch(eng, h, 1, "h")
    i = Batch(eng, model, 125, [(5 * o, 30, 1) for o in range(20)], L, [([40, 41, 42, 90, 91], [])] * 3, 125)
    assert i.fx.R == 20 and (i.s.det.sum(1) == 5).all()
    assert not model.windows_alone(i.s, i.fx.off, i.fx.nss, propagate=True).any()
    one_launch(eng, i, 1, "i")
    j = Batch(eng, model, 30, [(0, 30, 6)], L, [(list(range(0, 25, 4)), [])], 30)
    assert j.s.miss.sum() == 7 and j.s.status.tolist() == [SINGULAR]
    one_launch(eng, j, 1, "j")


def test_one_column_one_repair(eng, model):
    """(k) K 1, R 1, L 4: the tile of one unknown"""
    k = Batch(eng, model, 1, [(0, 1, 1)], 4, [([0], []), ([], []), ([0], [0])], 1)
    assert k.s.status.tolist() == [RECOVERED, NOTHING, NOTHING]
    one_launch(eng, k, 1, "k")


def test_shapes_and_knobs_that_keep_the_separate_launches(eng, model):
    """K = R = 128 does not fit LDS; knob plan != 0 forces the separate launches: the counter does not move"""
    big = Batch(eng, model, 128, [(0, 128, 128)], 64, [(list(range(0, 120, 3)), list(range(100, 128)))] * 2, 129)
    assert (big.s.det.sum(1) == 40).all()
    one_launch(eng, big, 0, "K = R = 128")
    b3 = five_windows(eng, model, 64, [A, B, C_], 55)
    with knob(eng, "plan", 1):
        one_launch(eng, b3, 0, "plan 1")
    one_launch(eng, b3, 1, "plan 0 again")


@pytest.mark.parametrize("L", [36, 1200])
def test_knobs_and_streams_give_the_same_bytes(eng, model, L):
    """plan 1 (the separate launches) and span_compact 0 (the full setup in the one launch) write what the
    default writes, byte for byte; so does a call on a caller's non-default stream."""
    batches = [five_windows(eng, model, L, [A, B, C_, D, E] * 2, 56),
               Batch(eng, model, 64, [(0, 64, 12)], L, tile_patterns(), 66, zero=[(3, 9)]),
               Batch(eng, model, 125, [(5 * o, 30, 1) for o in range(20)], L, [([40, 41, 42, 90, 91], [])], 126)]
    for bt in batches:
        ref = one_launch(eng, bt, 1, "default")
        with knob(eng, "plan", 1):
            got = one_launch(eng, bt, 0, "plan 1")
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))
        with knob(eng, "span_compact", 0):
            got = one_launch(eng, bt, 1, "span_compact 0")
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))
        side = torch.cuda.Stream()
        before = eng.span_one_launch_calls()
        got = bt.run(eng, stream=side)
        assert eng.span_one_launch_calls() - before == 1
        bt.check(got, "side stream")
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))
