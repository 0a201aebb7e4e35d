"""Full-rank RLC recovery on the row paths (fecgpu_rlc_decode_rows_full / _rows_fused_full and their host
forms) and inside the one-block kernels that small batches of fecgpu_rlc_decode_full take.  Bit-exact:
patterns and verdicts come from decode_full_cases.py (a CPU rank routine that asks the engine nothing),
recovered bytes are compared with the original sources, and every comparison covers the whole pool the
rows lie in, so a byte written to a present row, to a row of a singular block or past a row fails it."""
import numpy as np
import pytest

from decode_full_cases import RECOVERED, REF_UB, SINGULAR, TUPLES, case, damaged, gf_rank, masks, rows_for
from oracle_py import Oracle, synth_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
SENTINEL = 0xC3
GAP = 16  # sentinel bytes behind every row


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(0)


def to_dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kmask(k):
    return np.array([(1 << min(k, 64)) - 1, (1 << max(k - 64, 0)) - 1], np.uint64)


def seeds_of(nb, r):
    return ((np.arange(nb, dtype=np.uint32)[:, None] << 8) | np.arange(r, dtype=np.uint32)[None, :]).reshape(-1)


def new_out(nb):
    return (torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV),
            torch.full((nb, 2), -1, dtype=torch.int64, device=DEV))


def host_out(t):
    return t[0].cpu().numpy(), t[1].cpu().numpy().view(np.uint64)


def packed_full(eng, c, work, rep, seeds):
    """fecgpu_rlc_decode_full with rep_seed on the packed rows: rows, status, masks."""
    nb = work.shape[0]
    w, out = to_dev(work), new_out(nb)
    eng.rlc_decode_full(w, to_dev(rep), to_dev(c.sp[:nb]), to_dev(c.rp[:nb]), *out, c.k, c.r, work.shape[2],
                        nblocks=nb, rep_seed=to_dev(seeds))
    torch.cuda.synchronize()
    return (w.cpu().numpy(),) + host_out(out)


def selected(c):
    """sel[b][x]: full mode selects the x-th received repair of block b -- the lowest-index independent set
    (a repair is taken iff it raises the rank of the ones before it).  CPU only."""
    o = Oracle()
    rows = rows_for(lambda b, i: o.seed(b, i), c.k, c.miss, c.present)
    prev = np.zeros(c.nb, np.int64)
    sel = np.zeros((c.nb, c.p), bool)
    for x in range(c.p):
        rk = gf_rank(rows[:, :x + 1])
        sel[:, x] = rk > prev
        prev = rk
    return sel


class Pool:
    """Every row of a batch at its own place in one byte pool, in shuffled order, 4-byte aligned, with GAP
    sentinel bytes behind it (and up to 3 more up to the next aligned offset)."""

    def __init__(self, rng, lens):
        lens = np.asarray(lens, np.int64)
        order = rng.permutation(lens.size)
        self.off = np.zeros(lens.size, np.int64)
        o = 0
        for x in order:
            self.off[x] = o
            o += ((int(lens[x]) + 3) & ~3) + GAP
        self.lens = lens
        self.size = o
        self.bytes = np.full(o, SENTINEL, np.uint8)

    def put(self, x, row):
        self.bytes[self.off[x]:self.off[x] + len(row)] = row


def row_pool(c, work, rep, src_len, rep_len, seed):
    """The batch's k + r rows per block shuffled through one pool: sources first (block-major), then repairs.
    Row x holds src_len / rep_len bytes of its packed row."""
    nb, k, r = work.shape[0], c.k, c.r
    rng = np.random.default_rng(seed)
    p = Pool(rng, np.concatenate([src_len.reshape(-1), rep_len.reshape(-1)]))
    for b in range(nb):
        for j in range(k):
            p.put(b * k + j, work[b, j, :src_len[b, j]])
        for i in range(r):
            p.put(nb * k + b * r + i, rep[b, i, :rep_len[b, i]])
    return p


def tables(p, base, nb, k, r):
    addr = (p.off + base).astype(np.uint64)
    return addr[:nb * k].copy(), addr[nb * k:].copy()


# ------------------------------------------------------------------------------------------ row forms
CASES_ROWS = {"A": (TUPLES[0], None, dict(give_up=29, singular=10, later=0)),
              "B": (TUPLES[1], 512, dict(give_up=7, singular=0, later=3))}


def _case_rows(name):
    tup, cut, counts = CASES_ROWS[name]
    c = case(*tup, 64, cut=cut)
    assert int(((c.ref_st == REF_UB) & c.full).sum()) == counts["give_up"]
    assert int((~c.full).sum()) == counts["singular"]
    assert int((c.full & ~c.first).sum()) == counts["later"]
    return c


@pytest.mark.parametrize("name", ["A", "B"])
def test_rows_full(eng, name):
    c = _case_rows(name)
    nb, k, r, L = c.nb, c.k, c.r, c.L
    work, rep = damaged(c)
    seeds = seeds_of(nb, r)
    full_len = lambda n: np.full(n, L, np.int64)  # noqa: E731
    p = row_pool(c, work, rep, full_len((nb, k)), full_len((nb, r)), [7, nb])
    exp_st = np.where(c.full, RECOVERED, SINGULAR).astype(np.uint8)
    exp_rec = np.where(c.full[:, None], ~c.sp & kmask(k)[None, :], np.uint64(0))
    want = p.bytes.copy()
    for b in np.nonzero(c.full)[0]:
        for j in c.miss[b]:
            want[p.off[b * k + j]:p.off[b * k + j] + L] = c.src[b, j]
    # every present row untouched, every row of a SINGULAR block still its 0xA5 fill, sentinels intact
    for b in np.nonzero(~c.full)[0]:
        for j in c.miss[b]:
            assert (want[p.off[b * k + j]:p.off[b * k + j] + L] == 0xA5).all()
    sel = selected(c)
    results = []
    for zero_unused in (False, True):
        pool = to_dev(p.bytes)
        srow, rrow = tables(p, pool.data_ptr(), nb, k, r)
        if zero_unused:  # absent and unselected repairs, and every row of a singular block: never dereferenced
            keep = np.zeros((nb, r), bool)
            for b in range(nb):
                keep[b, c.present[b][sel[b]]] = c.full[b]
            assert (keep.sum(axis=1)[c.full] == c.e).all() and keep.sum() < sum(len(x) for x in c.present)
            rrow[~keep.reshape(-1)] = 0
            srow.reshape(nb, k)[~c.full] = 0
        out = new_out(nb)
        eng.rlc_decode_rows_full(to_dev(srow), to_dev(rrow), to_dev(seeds), to_dev(c.sp), to_dev(c.rp), *out, nb, k,
                                 r, L)
        torch.cuda.synchronize()
        st, rec = host_out(out)
        got = pool.cpu().numpy()
        assert np.array_equal(st, exp_st), np.nonzero(st != exp_st)[0][:10]
        assert np.array_equal(rec, exp_rec)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        results.append((st, rec, got))
    # and the packed full decode on the same rows
    g, st_p, rec_p = packed_full(eng, c, work, rep, seeds)
    assert np.array_equal(st_p, exp_st) and np.array_equal(rec_p, exp_rec)
    assert np.array_equal(g[c.full], c.src[c.full]) and np.array_equal(g[~c.full], work[~c.full])


# ------------------------------------------------------------------------------------------ fused form
def _ragged(c, seed):
    """Ragged lengths for the blocks of c: blk_len in 1..L with every residue mod 4, src_len <= blk_len with
    some 0; the sources cut to their lengths and the repairs of those sources."""
    rng = np.random.default_rng(seed)
    nb, k, L = c.nb, c.k, c.L
    blk = rng.integers(1, L + 1, nb)
    blk[:8] = [1, 2, 3, 5, 6, 7, L, L - 1]
    assert {int(x) % 4 for x in blk} == {0, 1, 2, 3}
    src_len = np.zeros((nb, k), np.int64)
    for b in range(nb):
        n = rng.integers(0, int(blk[b]) + 1, k)
        n[rng.integers(0, k)] = blk[b]
        if b % 5 == 0:
            n[rng.integers(0, k)] = 0
        src_len[b] = n
    assert (src_len == 0).any()
    src = c.src.copy()
    src[np.arange(L)[None, None, :] >= src_len[:, :, None]] = 0
    rep = Oracle().rlc_encode_batch(src, c.r, 0)
    assert not rep[np.arange(L)[None, None, :] >= blk[:, None, None].repeat(c.r, 1)].any()
    return blk, src_len, src, rep


@pytest.mark.parametrize("name", ["E", "A1024"])
def test_rows_fused_full(eng, name):
    if name == "E":
        c = case(*TUPLES[4], 36, cut=512)
        assert int(((c.ref_st == REF_UB) & c.full).sum()) == 6 and int((~c.full).sum()) == 0
        assert int((c.full & ~c.first).sum()) == 4
    else:
        c = case(*TUPLES[0], 64, cut=1024)
        assert int(((c.ref_st == REF_UB) & c.full).sum()) == 7 and int((~c.full).sum()) == 1
    nb, k, r, L = c.nb, c.k, c.r, c.L
    blk, src_len, src, rep_all = _ragged(c, [3, nb])
    miss = np.zeros((nb, k), bool)
    for b in range(nb):
        miss[b, c.miss[b]] = True
    work = src.copy()
    work[miss] = 0xA5
    rep = rep_all.copy()
    for b in range(nb):
        rep[b, np.setdiff1d(np.arange(r), c.present[b])] = 0x5C
    # a missing source's row has room for the block's length; an absent repair's row is never read
    slen_pool = np.where(miss, blk[:, None], src_len)
    rlen = np.repeat(blk[:, None], r, 1)
    p = row_pool(c, work, rep, slen_pool, rlen, [5, nb])
    pool = to_dev(p.bytes)
    srow, rrow = tables(p, pool.data_ptr(), nb, k, r)
    seeds = seeds_of(nb, r)
    out = new_out(nb)
    eng.rlc_decode_rows_fused_full(to_dev(srow), to_dev(np.where(miss, 0, src_len).astype(np.uint32).reshape(-1)),
                                   to_dev(rrow), to_dev(rlen.astype(np.uint32).reshape(-1)),
                                   to_dev(blk.astype(np.uint32)), to_dev(seeds), to_dev(c.sp), to_dev(c.rp), *out, nb,
                                   k, r, L)
    torch.cuda.synchronize()
    st, rec = host_out(out)
    got = pool.cpu().numpy()
    # the zero-padded packed full decode: status, masks and bytes
    work_p = work.copy()
    g, st_p, rec_p = packed_full(eng, c, work_p, rep, seeds)
    exp_st = np.where(c.full, RECOVERED, SINGULAR).astype(np.uint8)
    assert np.array_equal(st_p, exp_st)
    assert np.array_equal(st, st_p) and np.array_equal(rec, rec_p)
    nonzero = src.any(axis=2)
    exp_rec = masks(nb, [[j for j in c.miss[b] if c.full[b] and nonzero[b, j]] for b in range(nb)])
    assert np.array_equal(rec, exp_rec)
    want = p.bytes.copy()
    free = np.zeros(p.size, bool)  # bytes the fused form may or may not have written (fecgpu.h): all-zero sources
    for b in np.nonzero(c.full)[0]:
        for j in c.miss[b]:
            o, n = p.off[b * k + j], int(blk[b])
            want[o:o + n] = src[b, j, :n]  # exactly blk_len bytes, the sentinel behind them intact
            assert np.array_equal(g[b, j, :n], src[b, j, :n])
            if not nonzero[b, j]:
                free[o:o + n] = True
    bad = (got != want) & ~(free & (got == 0xA5))
    assert not bad.any(), np.flatnonzero(bad)[:8]


# ------------------------------------------------------------------------------------------ host forms
@pytest.mark.parametrize("cfg", ["pageable", "pinned", "mixed", "sub_batches"])
def test_rows_host_full(eng, cfg):
    from pquic_amd import HostPath
    c = _case_rows("B")
    nb, k, r, L = c.nb, c.k, c.r, c.L
    work, rep = damaged(c)
    seeds = seeds_of(nb, r)
    ones = lambda n: np.full(n, L, np.int64)  # noqa: E731
    p = row_pool(c, work, rep, ones((nb, k)), ones((nb, r)), [9, nb])
    # the device results
    pool = to_dev(p.bytes)
    srow, rrow = tables(p, pool.data_ptr(), nb, k, r)
    out = new_out(nb)
    eng.rlc_decode_rows_full(to_dev(srow), to_dev(rrow), to_dev(seeds), to_dev(c.sp), to_dev(c.rp), *out, nb, k, r, L)
    torch.cuda.synchronize()
    st_d, rec_d = host_out(out)
    got_d = pool.cpu().numpy()
    assert np.array_equal(st_d, np.where(c.full, RECOVERED, SINGULAR))
    hp = HostPath(0, 3, (1 << 14) if cfg == "sub_batches" else (64 << 20))
    keep = []

    def arr(a, pin):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        if not pin:
            return a.copy()
        t = torch.from_numpy(a.copy()).pin_memory()
        keep.append(t)
        return t.numpy()

    pin = cfg in ("pinned", "mixed", "sub_batches")
    for fused in (False, True):
        pool = to_dev(p.bytes)
        srow, rrow = tables(p, pool.data_ptr(), nb, k, r)
        a = dict(srow=arr(srow, pin), rrow=arr(rrow, pin), seeds=arr(seeds, pin and cfg != "mixed"),
                 sp=arr(c.sp, pin), rp=arr(c.rp, pin), st=arr(np.full(nb, 0xEE, np.uint8), pin),
                 rec=arr(np.full((nb, 2), 0xFF, np.uint64), pin))
        if fused:
            lens = dict(sl=arr(np.full(nb * k, L, np.uint32), pin), rl=arr(np.full(nb * r, L, np.uint32), pin),
                        bl=arr(np.full(nb, L, np.uint32), pin))
            hp.rlc_decode_rows_fused_full(a["srow"], lens["sl"], a["rrow"], lens["rl"], lens["bl"], a["seeds"],
                                          a["sp"], a["rp"], a["st"], a["rec"], nb, k, r, L)
        else:
            hp.rlc_decode_rows_full(a["srow"], a["rrow"], a["seeds"], a["sp"], a["rp"], a["st"], a["rec"], nb, k, r, L)
        torch.cuda.synchronize()
        assert np.array_equal(a["st"], st_d), (cfg, fused)
        assert np.array_equal(a["rec"].view(np.uint64).reshape(nb, 2), rec_d), (cfg, fused)
        assert np.array_equal(pool.cpu().numpy(), got_d), (cfg, fused)
    hp.close()


# ------------------------------------------------------------------------------------------ one-block kernels
def _one_block_set(tup, L):
    """The blocks of a tuple that reference mode gives up on but the received repairs determine, its singular
    blocks and two blocks reference mode recovers."""
    c = case(*tup, L)
    give_up = np.nonzero((c.ref_st == REF_UB) & c.full)[0]
    singular = np.nonzero(~c.full)[0]
    ref_ok = np.nonzero(c.ref_st == RECOVERED)[0][:2]
    return c, give_up, singular, ref_ok


ONE_BLOCK = {"A": (TUPLES[0], 1200, 29, 10), "C": (TUPLES[2], 64, 44, 6), "D": (TUPLES[3], 64, 34, 3)}


def _run_packed(eng, c, idx, work, rep, mode):
    nb = idx.size
    w, out = to_dev(work), new_out(nb)
    args = (w, to_dev(rep), to_dev(c.sp[idx]), to_dev(c.rp[idx]), *out, c.k, c.r, c.L)
    if mode == "full":
        eng.rlc_decode_full(*args, nblocks=nb, fbn=to_dev(idx.astype(np.uint32)))
    else:
        eng.rlc_decode(*args, nblocks=nb, fbn=to_dev(idx.astype(np.uint32)))
    torch.cuda.synchronize()
    return (w.cpu().numpy(),) + host_out(out)


@pytest.mark.parametrize("name", ["A", "C", "D"])
@pytest.mark.parametrize("nb", [1, 3, 64, 65])
def test_one_block_kernels_full(eng, name, nb):
    """EM 4 (A), 8 (C) and 16 (D, the LDS wave plan): the in-kernel re-plan of the one-launch path (defaults:
    the rows in LDS) against plan + fix-up + apply, reached by rule (small_lds 0) and by force (plan 1)."""
    tup, L, n_give_up, n_singular = ONE_BLOCK[name]
    c, give_up, singular, ref_ok = _one_block_set(tup, L)
    assert give_up.size == n_give_up and singular.size == n_singular and ref_ok.size == 2
    pick = np.concatenate([give_up, singular, ref_ok])
    # batches of nb: walk the set so that every batch size sees blocks of all three kinds
    order = np.concatenate([give_up[:1], singular[:1], ref_ok[:1], pick])
    idx = order[np.arange(nb) % order.size] if nb > 1 else give_up[:1]
    work_all, rep_all = damaged(c)
    work, rep = work_all[idx], rep_all[idx]
    exp_st = np.where(c.full[idx], RECOVERED, SINGULAR).astype(np.uint8)
    exp_rec = np.where(c.full[idx][:, None], ~c.sp[idx] & kmask(c.k)[None, :], np.uint64(0))
    want = np.where(c.full[idx][:, None, None], c.src[idx], work)
    runs = {}
    runs["defaults"] = _run_packed(eng, c, idx, work, rep, "full")
    with eng.knob("small_lds", 0):
        runs["small_lds 0"] = _run_packed(eng, c, idx, work, rep, "full")
    with eng.knob("plan", 1):
        runs["plan 1"] = _run_packed(eng, c, idx, work, rep, "full")
    for tag, (g, st, rec) in runs.items():
        assert np.array_equal(st, exp_st), (tag, st, exp_st)
        assert np.array_equal(rec, exp_rec), tag
        assert np.array_equal(g, want), (tag, np.nonzero((g != want).any(axis=(1, 2)))[0][:8])
    # reference mode afterwards is what it was
    _, st_ref, _ = _run_packed(eng, c, idx, work, rep, "ref")
    assert np.array_equal(st_ref, c.ref_st[idx])
    assert (st_ref[np.isin(idx, give_up)] == REF_UB).all()


def test_one_block_kernels_clear_dependency_flags(eng):
    """The zero-symbol shapes of test_full_decode_zero_symbol (k8 r4, 16 blocks) through the one-launch path
    and through plan + fix-up + apply: equal status, masks and bytes, and the symbol beside the zero one is
    reported whichever of the two is zero -- so the dependency flags are cleared inside the kernel."""
    k, r, L, nb = 8, 4, 64, 16
    rng = np.random.default_rng(k)
    miss = [np.array(sorted(rng.choice(k, 2, replace=False))) for _ in range(nb)]
    zero = [int(miss[b][b & 1]) for b in range(nb)]

    class Z:
        pass
    c = Z()
    c.k, c.r, c.e, c.nb, c.L = k, r, 2, nb, L
    c.miss = miss
    c.present = [np.array(sorted(rng.choice(r, 2 + b % 3, replace=False))) for b in range(nb)]
    c.src = synth_bytes(nb * k * L, 99 + k).reshape(nb, k, L).copy()
    for b in range(nb):
        c.src[b, zero[b]] = 0
    o = Oracle()
    c.rep = o.rlc_encode_batch(c.src, r, 0)
    c.sp = masks(nb, [[j for j in range(k) if j not in set(m.tolist())] for m in miss])
    c.rp = masks(nb, c.present)
    full = np.array([gf_rank(rows_for(lambda _, i, b=b: o.seed(b, i), k, [miss[b]], [c.present[b]]))[0] == 2
                     for b in range(nb)])
    assert full.sum() >= nb - 2
    work, rep = damaged(c)
    idx = np.arange(nb)
    runs = {"defaults": _run_packed(eng, c, idx, work, rep, "full")}
    with eng.knob("small_lds", 0):
        runs["small_lds 0"] = _run_packed(eng, c, idx, work, rep, "full")
    with eng.knob("plan", 1):
        runs["plan 1"] = _run_packed(eng, c, idx, work, rep, "full")
    g1, st1, rec1 = runs["plan 1"]
    assert np.array_equal(st1, np.where(full, RECOVERED, SINGULAR))
    for b in np.nonzero(full)[0]:
        other = int(miss[b][1 - (b & 1)])
        assert [j for j in range(k) if (int(rec1[b, 0]) >> j) & 1] == [other], b
        assert np.array_equal(g1[b], c.src[b]), b
    for tag in ("defaults", "small_lds 0"):
        g, st, rec = runs[tag]
        assert np.array_equal(st, st1) and np.array_equal(rec, rec1) and np.array_equal(g, g1), tag
