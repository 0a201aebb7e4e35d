"""The compacted span data pass (knob span_compact) on the device.  Every case runs with the knob at 0 and at
1 on the same inputs: both runs must equal the numpy model (span_model.py; status, recovered[], every row,
rows the model does not mark determined untouched) and each other, byte for byte.  The helpers and fixtures of
test_span_decode_gpu.py build the spans."""
import contextlib

import numpy as np
import pytest

from span_model import RECOVERED, SpanModel, pack
from test_span_decode_gpu import (MISSING, SENTINEL, Pool, Spans, check, damaged, host_out, new_out, random_losses,
                                  run_packed, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(0)


@pytest.fixture(scope="module")
def model():
    return SpanModel()


@contextlib.contextmanager
def knob(eng, name, value):
    old = eng.get_knob(name)
    eng.set_knob(name, value)
    try:
        yield
    finally:
        eng.set_knob(name, old)


def both(eng, run):
    """run() with span_compact 0 and 1; every array of the two results must be identical."""
    out = []
    for v in (0, 1):
        with knob(eng, "span_compact", v):
            out.append(run())
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    return out[1]


def packed(eng, model, fx, present, rpresent):
    def run():
        _, _, _, got, st, rec = run_packed(eng, model, fx, present, rpresent)  # checks against the model
        return got, st, rec
    return both(eng, run)


# --------------------------------------------------------------------------------- padded groups (packed form)
@pytest.mark.parametrize("L,nb", [(64, 65), (64, 1), (4, 4100)])
def test_padded_groups(eng, model, L, nb):
    """Spans of 16 columns from windows k6 r1 step 2, losses drawn per span: the blocks of a group list
    different numbers of inputs, so the shorter lists are padded to the group's longest."""
    fx = Spans(16, L, nb, [(2 * w, 6, 1) for w in range(6)], data_seed=L + nb)
    present, rpresent = random_losses(fx, [L, nb], 0.15, 0.1)
    present[0, [3, 4]] = False  # span 0: two losses in the first windows
    present[0, 5:] = True
    rpresent[0] = True
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, pack(present), pack(rpresent))
    if nb > 1:
        n = s.det.sum(1)
        assert len(set(n[s.status == RECOVERED].tolist())) >= 3  # groups mix blocks of different sizes
    packed(eng, model, fx, present, rpresent)


# --------------------------------------------------------------------------------- tile counts (packed form)
def _spread(R):
    """R windows of 16 columns spread over a span of 64, one repair each"""
    return [(w * 48 // max(R - 1, 1), 16, 1) for w in range(R)]


WIDE16 = [(4 * w, 16, 1) for w in range(13)] + [(0, 64, 3)]  # K 64, R 16


def _tile_case(model, windows, e, seed):
    fx = Spans(64, 1200, 12, windows, data_seed=seed)
    rng = np.random.default_rng([seed, e])
    present = np.ones((fx.nb, fx.K), bool)
    rpresent = np.ones((fx.nb, fx.R), bool)
    for b in range(fx.nb):
        n = e if b % 2 == 0 else int(rng.integers(1, e + 3))
        present[b, rng.choice(64, n, replace=False)] = False
    rpresent[1::4, 0] = False
    return fx, present, rpresent


@pytest.mark.parametrize("e", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("layout", ["R16", "R16_noring", "Rtile"])
def test_tile_counts(eng, model, e, layout):
    """e lost sources per span at K 64, L 1200.  R16: 16 repair slots (the 16-unknown tile: the LDS ring by
    default, the register-prefetch kernel with knob ring 0).  Rtile: as many repairs as the tile of e unknowns
    holds, from windows of 16 columns, so the tiles of 1, 2, 4 and 8 unknowns run."""
    if layout == "Rtile":
        R = {1: 1, 2: 2, 3: 4, 4: 4, 8: 8}[e]
        fx, present, rpresent = _tile_case(model, _spread(R), e, 100 + e)
        offs = [o for o, _, _ in fx.windows]
        for b in range(0, fx.nb, 2):  # one loss under each of e windows: determined
            present[b] = True
            present[b, [offs[w] + 2 + (w % 3) for w in range(e)]] = False
            rpresent[b] = True
    else:
        fx, present, rpresent = _tile_case(model, WIDE16, e, 200 + e)
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, pack(present), pack(rpresent))
    if layout == "Rtile":
        assert (s.det.sum(1)[::2] == e).all(), s.det.sum(1)
    with knob(eng, "ring", 0 if layout == "R16_noring" else 2):
        packed(eng, model, fx, present, rpresent)


@pytest.mark.parametrize("layout", ["R16_noring", "R2"])
def test_far_apart_losses_need_the_whole_span(eng, model, layout):
    """Two losses at the two ends under repairs that cover the whole span: the tile's inputs are all of it."""
    windows = WIDE16 if layout != "R2" else [(0, 64, 2)]
    fx = Spans(64, 1200, 5, windows, data_seed=31)
    present = np.ones((fx.nb, fx.K), bool)
    present[:, [1, 62]] = False
    present[3, [20, 40]] = False
    rpresent = np.ones((fx.nb, fx.R), bool)
    if layout != "R2":
        rpresent[:, :13] = False  # only the three full-width repairs
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, pack(present), pack(rpresent))
    assert s.det[0, 1] and s.det[0, 62]
    with knob(eng, "ring", 0 if layout == "R16_noring" else 2):
        packed(eng, model, fx, present, rpresent)


@pytest.mark.parametrize("layout", ["R16_noring", "R8"])
def test_single_loss_in_the_first_window(eng, model, layout):
    """One loss that only the first window covers: at most its 16 rows are inputs."""
    fx = Spans(64, 1200, 5, WIDE16[:13] + [(40, 24, 3)] if layout != "R8" else _spread(8), data_seed=32)
    present = np.ones((fx.nb, fx.K), bool)
    present[:, 2] = False
    rpresent = np.ones((fx.nb, fx.R), bool)
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, pack(present), pack(rpresent))
    assert s.det[:, 2].all() and s.selected.sum(1).tolist() == [1] * fx.nb and s.selected[:, 0].all()
    with knob(eng, "ring", 0 if layout == "R16_noring" else 2):
        packed(eng, model, fx, present, rpresent)


def test_ring_tiles_ignore_the_knob(eng, model):
    """More than 8 unknowns at K 64, L 1200 take the LDS-ring kernel, which keeps its own setup."""
    fx, present, rpresent = _tile_case(model, WIDE16, 12, 300)
    with knob(eng, "span_compact", 1):
        run_packed(eng, model, fx, present, rpresent)


# --------------------------------------------------------------------------------- row form
def run_rows(eng, model, fx, present, rpresent, blk=None, src_len=None, rep_len=None, host=None):
    """fecgpu_rlc_span_decode_rows_fused (or its host form) on the rows of fx shuffled through one pool, with
    the knob at 0 and 1; checked against the model."""
    nb, K, R, L = fx.nb, fx.K, fx.R, fx.L
    blk = np.full(nb, L) if blk is None else blk
    src_len = np.full((nb, K), L) if src_len is None else src_len
    rep_len = np.full((nb, R), L) if rep_len is None else rep_len
    sp, rp = pack(present), pack(rpresent)
    s = model.solve(K, fx.seed, fx.off, fx.nss, sp, rp)
    p = Pool(fx, s, blk, src_len, rep_len, fx.encode(eng), 7)
    slen = np.where(s.miss, 0, src_len).astype(np.uint32).reshape(-1)
    rlen = np.where(s.selected, rep_len, L).astype(np.uint32).reshape(-1)
    exp_rec = model.recovered(s, fx.src)
    keep = []

    def arr(a, pin):
        a = np.ascontiguousarray(a)
        a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
        if not pin:
            return a.copy()
        t = torch.from_numpy(a.copy()).pin_memory()
        keep.append(t)
        return t.numpy()

    def run():
        pool = to_dev(p.bytes)
        srow, rrow = p.tables(pool.data_ptr())
        if host is None:
            out = new_out(nb)
            eng.rlc_span_decode_rows_fused(to_dev(srow), to_dev(slen), to_dev(rrow), to_dev(rlen),
                                           to_dev(blk.astype(np.uint32)), to_dev(fx.seed), to_dev(fx.off),
                                           to_dev(fx.nss), to_dev(sp), to_dev(rp), *out, nb, K, R, L)
            torch.cuda.synchronize()
            st, rec = host_out(out)
        else:
            a = [arr(srow, True), arr(slen, True), arr(rrow, True), arr(rlen, True), arr(blk.astype(np.uint32), True),
                 arr(fx.seed, True), arr(fx.off, True), arr(fx.nss, False), arr(sp, True), arr(rp, True),
                 arr(np.full(nb, 0xEE, np.uint8), True), arr(np.full((nb, 2), 0xFF, np.uint64), True)]
            host.rlc_span_decode_rows_fused(*a, nb, K, R, L)
            torch.cuda.synchronize()
            st, rec = a[10].copy(), a[11].view(np.uint64).reshape(nb, 2).copy()
        got = pool.cpu().numpy()
        assert np.array_equal(st, s.status), np.nonzero(st != s.status)[0][:10]
        assert np.array_equal(rec, exp_rec), np.nonzero((rec != exp_rec).any(1))[0][:10]
        assert np.array_equal(got, p.want), np.flatnonzero(got != p.want)[:8]
        return st, rec, got

    both(eng, run)
    return s


def _ragged(nb=48, K=60, cover=55, L=1200):
    """Ragged symbols of length 0..blk under windows k30 r1 step 5 on the first `cover` columns; the trailing
    columns are padding: present, length 0, under no repair."""
    fx = Spans(K, L, nb, [(5 * w, 30, 1) for w in range((cover - 30) // 5 + 1)], data_seed=41)
    rng = np.random.default_rng(41)
    blk = rng.integers(1, L + 1, nb)
    blk[:8] = [1, 2, 3, 5, 6, 7, L, L - 1]
    src_len = rng.integers(0, blk[:, None] + 1, (nb, K))
    src_len[np.arange(nb), rng.integers(0, cover, nb)] = blk
    src_len[:, cover:] = 0
    src_len[:, 7] = 0  # a zero-length present row under the windows
    fx.src[np.arange(L)[None, None, :] >= src_len[:, :, None]] = 0
    rep_len = np.stack([src_len[:, o:o + n].max(1) for o, n, r in fx.windows for _ in range(r)], 1)
    present, rpresent = random_losses(fx, 6, 0.07, 0.15)
    present[:, cover:] = True
    present[:, 7] = True
    present[:8, 26] = False
    return fx, blk, src_len, rep_len, present, rpresent


def test_rows_ragged_with_padding_columns(eng, model):
    fx, blk, src_len, rep_len, present, rpresent = _ragged()
    s = run_rows(eng, model, fx, present, rpresent, blk, src_len, rep_len)
    assert s.det.any(1).sum() >= 20 and (src_len[~s.miss] == 0).any()


@pytest.mark.parametrize("K,k,r,step", [(125, 30, 1, 5), (128, 32, 8, 8)])
def test_rows_wide_spans(eng, model, K, k, r, step):
    """K 125 R 20 from k30 r1 step 5 windows and K 128 R 104 from k32 r8 step 8 windows at p = 0.10"""
    fx = Spans(K, 1200, 65, [(step * w, k, r) for w in range((K - k) // step + 1)], data_seed=K)
    assert fx.R == (20 if K == 125 else 104)
    present, rpresent = random_losses(fx, K, 0.10, 0.10)
    s = run_rows(eng, model, fx, present, rpresent)
    assert s.det.any(1).sum() >= 40


@pytest.mark.parametrize("nb", [1, 65])
def test_rows_two_chunks(eng, model, nb):
    fx = Spans(55, 2052, nb, [(5 * w, 30, 1) for w in range(6)], data_seed=nb)
    present, rpresent = random_losses(fx, 2052 + nb, 0.08, 0.1)
    present[0] = True
    present[0, [25, 27]] = False
    rpresent[0] = True
    s = run_rows(eng, model, fx, present, rpresent)
    assert s.det[0, 25] and s.det[0, 27]


def test_rows_more_than_16_unknowns(eng, model):
    """Several tile launches and the finalize kernel"""
    fx = Spans(40, 1200, 12, [(0, 20, 10), (10, 30, 12)], data_seed=17)
    rng = np.random.default_rng(17)
    present = np.ones((fx.nb, fx.K), bool)
    for b in range(fx.nb):
        present[b, rng.choice(40, 17 + b % 5, replace=False)] = False
    rpresent = np.ones((fx.nb, fx.R), bool)
    rpresent[1::3, 4] = False
    s = run_rows(eng, model, fx, present, rpresent)
    assert (s.det.sum(1) > 16).sum() >= 6


def test_rows_host_form_with_a_pageable_table(eng, model):
    from pquic_amd import HostPath
    fx, blk, src_len, rep_len, present, rpresent = _ragged(nb=24)
    hp = HostPath(0, 3, 1 << 18)
    try:
        run_rows(eng, model, fx, present, rpresent, blk, src_len, rep_len, host=hp)
    finally:
        hp.close()


# --------------------------------------------------------------------------------- plan, then apply
def test_plan_then_apply(eng, model):
    nb, L = 70, 1200
    fx = Spans(55, L, nb, [(5 * w, 30, 1) for w in range(6)], data_seed=61)
    present, rpresent = random_losses(fx, 61, 0.08, 0.15)
    sp, rp = pack(present), pack(rpresent)
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, sp, rp)
    work, rep_w = damaged(fx, fx.encode(eng), s)
    exp_rec = model.recovered(s, fx.src)
    em = min(fx.K, fx.R)

    def run():
        ws = eng.alloc_workspace(nb, fx.K, fx.R)
        eng.rlc_span_decode_plan(to_dev(fx.seed), to_dev(fx.off), to_dev(fx.nss), to_dev(sp), to_dev(rp), fx.K, fx.R,
                                 nb, ws)
        w, r = to_dev(work), to_dev(rep_w)
        dst = torch.full((nb, fx.K, L), SENTINEL, dtype=torch.uint8, device=DEV)
        out = new_out(nb)
        eng.rlc_decode_apply_to(w, r, dst, *out, fx.K, fx.R, L, nb, ws)
        dpk = torch.full((nb, em, L), SENTINEL, dtype=torch.uint8, device=DEV)
        out2 = new_out(nb)
        eng.rlc_decode_apply_packed(w, r, dpk, *out2, fx.K, fx.R, L, nb, ws)
        torch.cuda.synchronize()
        st, rec = host_out(out)
        st2, rec2 = host_out(out2)
        assert np.array_equal(w.cpu().numpy(), work)
        return st, rec, dst.cpu().numpy(), st2, rec2, dpk.cpu().numpy()

    with knob(eng, "span_compact", 1):
        st, rec, d, st2, rec2, dp = run()
    for a, b in ((st, s.status), (st2, s.status), (rec, exp_rec), (rec2, exp_rec)):
        assert np.array_equal(a, b)
    assert np.array_equal(d[s.det], fx.src[s.det]) and (d[~s.det] == SENTINEL).all()
    for b in range(nb):
        cols = np.nonzero(s.det[b])[0]
        assert np.array_equal(dp[b, :cols.size], fx.src[b, cols]), b
        assert (dp[b, cols.size:] == SENTINEL).all(), b
    both(eng, run)


# --------------------------------------------------------------------------------- the other decode modes
def test_reference_and_full_rank_decode_do_not_see_the_knob(eng):
    """One block batch through the reference-faithful and the full-rank decode, knob at 0 and 1: same bytes."""
    nb, k, r, L = 70, 32, 8, 1200
    rng = np.random.default_rng(9)
    src = torch.from_numpy(rng.integers(0, 256, (nb, k, L), dtype=np.uint8)).to(DEV)
    rep = torch.empty((nb, r, L), dtype=torch.uint8, device=DEV)
    eng.rlc_encode(src, rep, k, r, L, fbn_base=3)
    present = np.ones((nb, k), bool)
    for b in range(nb):
        present[b, rng.choice(k, 1 + b % 8, replace=False)] = False
    rpresent = rng.random((nb, r)) < 0.9
    work_h = np.where(present[:, :, None], src.cpu().numpy(), np.uint8(MISSING))

    def run():
        res = []
        for full in (False, True):
            w = to_dev(work_h)
            out = new_out(nb)
            fn = eng.rlc_decode_full if full else eng.rlc_decode
            fn(w, rep, to_dev(pack(present)), to_dev(pack(rpresent)), *out, k, r, L, fbn_base=3)
            torch.cuda.synchronize()
            res += [*host_out(out), w.cpu().numpy()]
        return res

    res = both(eng, run)
    assert (res[3] == RECOVERED).sum() >= 20  # the full-rank run recovers
