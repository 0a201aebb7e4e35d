"""Full-rank RLC decode (fecgpu_rlc_decode_full) on the device.  Bit-exact: recovered bytes are
compared with the original sources, statuses with a CPU rank verdict (decode_full_cases.py) that
never asks the engine."""
import numpy as np
import pytest

from decode_full_cases import (NOTHING, RECOVERED, REF_UB, SINGULAR, TUPLES, bits, case, damaged, gf, gf_rank,
                               masks, rows_for)
from oracle_py import synth_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


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


def run(eng, c, work, rep, mode="full", fbn=None, rep_seed=None, sp=None, rp=None):
    """One decode call on copies of the damaged buffers (masks: the case's unless given); returns
    rows, status, masks."""
    nb = work.shape[0]
    w = to_dev(work)
    st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
    rec = torch.full((nb, 2), -1, dtype=torch.int64, device=DEV)
    a = (w, to_dev(rep))
    m = (to_dev(c.sp if sp is None else sp), to_dev(c.rp if rp is None else rp), st, rec)
    f = None if fbn is None else to_dev(fbn)
    if mode == "full":
        eng.rlc_decode_full(*a, *m, c.k, c.r, c.L, nblocks=nb, fbn=f,
                            rep_seed=None if rep_seed is None else to_dev(rep_seed))
    elif rep_seed is not None:
        eng.rlc_decode_seeded(*a, to_dev(rep_seed), *m, c.k, c.r, c.L, nblocks=nb)
    else:
        eng.rlc_decode(*a, *m, c.k, c.r, c.L, nblocks=nb, fbn=f)
    torch.cuda.synchronize()
    return w.cpu().numpy(), st.cpu().numpy(), rec.cpu().numpy().view(np.uint64)


def check_full(c, work, got, st, rec, full):
    """Status is the CPU verdict; recovered blocks hold the original sources and the mask of the
    missing set; singular blocks are untouched (their 0xA5 rows included) with an empty mask."""
    exp = np.where(full, RECOVERED, SINGULAR).astype(np.uint8)
    assert np.array_equal(st, exp), np.nonzero(st != exp)[0][:10]
    want = np.where(full[:, None, None], c.src, work)  # present rows untouched everywhere
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, bad[:10]
    miss_mask = ~c.sp & kmask(c.k)[None, :]
    exp_rec = np.where(full[:, None], miss_mask, np.uint64(0))
    assert np.array_equal(rec, exp_rec)


def check_against_reference_mode(got, st, rec, got_ref, st_ref, rec_ref):
    """Wherever reference mode recovers, full mode agrees in status, mask and bytes."""
    ok = st_ref == RECOVERED
    assert ok.any()
    assert np.array_equal(st[ok], st_ref[ok])
    assert np.array_equal(rec[ok], rec_ref[ok])
    assert np.array_equal(got[ok], got_ref[ok])


@pytest.mark.parametrize("k,r,e,p,nb,seed", TUPLES)
def test_full_decode_recovers_every_solvable_block(eng, k, r, e, p, nb, seed):
    """Every pattern of the batch: status = rank verdict, bytes = the original sources.  The batches
    are not vacuous: each holds blocks that reference mode gives up on and full mode recovers,
    singular blocks where no spare repair exists, and -- with spare repairs -- blocks solvable only
    through a repair beyond the first e received.  (100, 20, 20): multi-pass apply + finalize kernel."""
    c = case(k, r, e, p, nb, seed, 1200 if (k, r, e, p) == (16, 4, 4, 4) else 64)
    assert not (c.ref_st == NOTHING).any()
    assert int(((c.ref_st == REF_UB) & c.full).sum()) >= 15
    if p == e and k <= 64:
        assert int((~c.full).sum()) >= 3
    if p > e:
        assert int((c.full & ~c.first).sum()) >= 10
    work, rep = damaged(c)
    got, st, rec = run(eng, c, work, rep)
    assert not (st == REF_UB).any()
    check_full(c, work, got, st, rec, c.full)
    got_ref, st_ref, rec_ref = run(eng, c, work, rep, mode="ref")
    assert np.array_equal(st_ref, c.ref_st)  # the engine's reference mode is unchanged
    check_against_reference_mode(got, st, rec, got_ref, st_ref, rec_ref)


@pytest.mark.parametrize("nb", [1, 3, 64, 65])
def test_full_decode_small_batches_bypass_one_launch_paths(eng, nb):
    """The blocks of the first tuple that only full mode recovers, as batches small enough for
    fecgpu_rlc_decode's one-launch kernels (which plan in reference mode): all recovered."""
    c = case(*TUPLES[0], 1200)
    pick = np.nonzero((c.ref_st == REF_UB) & c.full)[0]
    assert pick.size >= 15
    idx = pick[np.arange(nb) % pick.size]
    work, rep = damaged(c)
    work, rep = work[idx], rep[idx]
    sel = dict(fbn=idx.astype(np.uint32), sp=c.sp[idx], rp=c.rp[idx])
    got, st, rec = run(eng, c, work, rep, **sel)
    assert (st == RECOVERED).all()
    assert np.array_equal(got, c.src[idx])
    assert np.array_equal(rec, ~c.sp[idx] & kmask(c.k)[None, :])
    _, st_ref, _ = run(eng, c, work, rep, mode="ref", **sel)
    assert (st_ref == REF_UB).all()


def test_full_decode_seeded_form(eng):
    """rep_seed[b * r + i] = i (the window framework's repairs carry block number 0): every block has the
    same coefficient rows, verified like the block-numbered form."""
    k, r, e, p, _, seed = TUPLES[1]
    nb, L = 512, 64
    c = case(k, r, e, p, TUPLES[1][4], seed, L, cut=nb)
    mul, _ = gf()
    rows = rows_for(lambda b, i: i, k, c.miss, c.present)
    full = gf_rank(rows) == e
    first = gf_rank(rows[:, :e]) == e
    assert (full & ~first).any()  # not vacuous: some block is solvable only through a later repair
    from oracle_py import Oracle
    o = Oracle()
    coef = np.stack([o.coefs(i, k) for i in range(r)])  # seed i == (0 << 8) | i
    rep = np.zeros((nb, r, L), np.uint8)
    for i in range(r):
        for j in range(k):
            rep[:, i] ^= mul[coef[i, j]][c.src[:, j]]

    class S:  # the same batch with the seeded repairs
        pass
    s = S()
    s.__dict__.update(c.__dict__)
    s.rep = rep
    work, repd = damaged(s)
    seeds = np.tile(np.arange(r, dtype=np.uint32), nb)
    got, st, rec = run(eng, s, work, repd, rep_seed=seeds)
    assert not (st == REF_UB).any()
    check_full(s, work, got, st, rec, full)
    got_ref, st_ref, rec_ref = run(eng, s, work, repd, mode="ref", rep_seed=seeds)
    check_against_reference_mode(got, st, rec, got_ref, st_ref, rec_ref)
    assert not ((st_ref == RECOVERED) & ~first).any()  # reference mode only ever takes the first e repairs


def test_full_decode_stages(eng):
    """rlc_decode_plan_full + apply / apply_to / apply_packed: the rows and masks of the one-call form."""
    k, r, e, p, _, seed = TUPLES[1]
    nb = 512
    c = case(k, r, e, p, TUPLES[1][4], seed, 64, cut=nb)
    assert (c.full & ~c.first).any() and ((c.ref_st == REF_UB) & c.full).any()
    work, rep = damaged(c)
    got, st, rec = run(eng, c, work, rep)
    check_full(c, work, got, st, rec, c.full)
    sp, rp, repd = to_dev(c.sp), to_dev(c.rp), to_dev(rep)
    ws = eng.alloc_workspace(nb, k, r)
    new = lambda: (torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV),  # noqa: E731
                   torch.full((nb, 2), -1, dtype=torch.int64, device=DEV))
    # in place
    w, (s1, r1) = to_dev(work), new()
    eng.rlc_decode_plan_full(sp, rp, k, r, nb, ws)
    eng.rlc_decode_apply(w, repd, s1, r1, k, r, c.L, nb, ws)
    torch.cuda.synchronize()
    assert np.array_equal(w.cpu().numpy(), got)
    assert np.array_equal(s1.cpu().numpy(), st) and np.array_equal(r1.cpu().numpy().view(np.uint64), rec)
    # to another buffer of src's layout: only recovered rows are written, src is only read
    w, (s2, r2) = to_dev(work), new()
    dst = torch.full((nb, k, c.L), 0x77, dtype=torch.uint8, device=DEV)
    eng.rlc_decode_plan_full(sp, rp, k, r, nb, ws)
    eng.rlc_decode_apply_to(w, repd, dst, s2, r2, k, r, c.L, nb, ws)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    assert np.array_equal(w.cpu().numpy(), work)
    assert np.array_equal(s2.cpu().numpy(), st) and np.array_equal(r2.cpu().numpy().view(np.uint64), rec)
    for b in range(nb):
        m = c.miss[b] if c.full[b] else []
        keep = np.setdiff1d(np.arange(k), m)
        assert np.array_equal(d[b, m], c.src[b, m]) and (d[b, keep] == 0x77).all(), b
    # packed: row u of block b = its u-th missing source
    (s3, r3) = new()
    dstp = torch.full((nb, min(k, r), c.L), 0x77, dtype=torch.uint8, device=DEV)
    eng.rlc_decode_plan_full(sp, rp, k, r, nb, ws)
    eng.rlc_decode_apply_packed(w, repd, dstp, s3, r3, k, r, c.L, nb, ws)
    torch.cuda.synchronize()
    d = dstp.cpu().numpy()
    assert np.array_equal(s3.cpu().numpy(), st) and np.array_equal(r3.cpu().numpy().view(np.uint64), rec)
    for b in np.nonzero(c.full)[0]:
        assert np.array_equal(d[b, :e], c.src[b, c.miss[b]]), b


@pytest.mark.parametrize("k,r", [(8, 4), (40, 20)])  # fused zero rule / multi-pass apply + finalize kernel
def test_full_decode_zero_symbol(eng, k, r):
    """One missing source is all zero, one is not: recovered, the zero row written as zeros with its bit
    clear, and -- unlike reference mode -- the other symbol inserted whichever of the two is zero."""
    L, nb = 64, 16
    rng = np.random.default_rng(k)
    miss = [np.array(sorted(rng.choice(k, 2, replace=False))) for _ in range(nb)]
    zero = [int(miss[b][b & 1]) for b in range(nb)]  # the lower / the higher missing source in turn

    class Z:
        pass
    c = Z()
    c.k, c.r, c.e, c.nb, c.L = k, r, 2, nb, L
    c.miss = miss
    c.present = [np.array(sorted(rng.choice(r, 2 + b % 3, replace=False))) for b in range(nb)]
    c.src = synth_bytes(nb * k * L, 99 + k).reshape(nb, k, L).copy()
    for b in range(nb):
        c.src[b, zero[b]] = 0
    from oracle_py import Oracle
    o = Oracle()
    c.rep = o.rlc_encode_batch(c.src, r, 0)
    c.sp = masks(nb, [[j for j in range(k) if j not in set(m.tolist())] for m in miss])
    c.rp = masks(nb, c.present)
    full = np.array([gf_rank(rows_for(lambda _, i, b=b: o.seed(b, i), k, [miss[b]], [c.present[b]]))[0] == 2
                     for b in range(nb)])
    assert full.sum() >= nb - 2
    work, rep = damaged(c)
    got, st, rec = run(eng, c, work, rep)
    assert np.array_equal(st, np.where(full, RECOVERED, SINGULAR))
    hidden = 0
    _, st_ref, rec_ref = run(eng, c, work, rep, mode="ref")
    for b in np.nonzero(full)[0]:
        other = int(miss[b][1 - (b & 1)])
        assert bits(rec[b], k) == [other], b
        assert np.array_equal(got[b], c.src[b]), b  # the zero row holds zeros, not the 0xA5 fill
        hidden += st_ref[b] == RECOVERED and bits(rec_ref[b], k) != [other]
    assert hidden > 0  # reference mode's zero rule does hide a symbol on some of these blocks


def test_full_decode_host_path(eng):
    """HostPath.rlc_decode_full on pageable and on page-locked arrays equals the device result."""
    from pquic_amd import HostPath
    k, r, e, p, _, seed = TUPLES[1]
    nb = 512
    c = case(k, r, e, p, TUPLES[1][4], seed, 64, cut=nb)
    work, rep = damaged(c)
    got, st, rec = run(eng, c, work, rep)
    check_full(c, work, got, st, rec, c.full)
    hp = HostPath(0, 3, 1 << 18)  # several sub-batches
    w = work.copy()
    st_h, rec_h = np.full(nb, 0xEE, np.uint8), np.full((nb, 2), 0xFF, np.uint64)
    hp.rlc_decode_full(w, rep, c.sp, c.rp, st_h, rec_h, nb, k, r, c.L)
    assert np.array_equal(w, got) and np.array_equal(st_h, st) and np.array_equal(rec_h, rec)
    pin = torch.from_numpy(work.copy()).pin_memory()
    rep_p = torch.from_numpy(rep).pin_memory()
    sp_p = torch.from_numpy(c.sp.view(np.int64)).pin_memory()
    rp_p = torch.from_numpy(c.rp.view(np.int64)).pin_memory()
    st_p = torch.full((nb,), 0xEE, dtype=torch.uint8).pin_memory()
    rec_p = torch.full((nb, 2), -1, dtype=torch.int64).pin_memory()
    hp.rlc_decode_full(pin, rep_p, sp_p, rp_p, st_p, rec_p, nb, k, r, c.L)
    assert np.array_equal(pin.numpy(), got) and np.array_equal(st_p.numpy(), st)
    assert np.array_equal(rec_p.numpy().view(np.uint64), rec)
    hp.close()


def test_full_decode_plan_knob(eng):
    """Whatever plan kernel the "plan" knob forces for the reference pass, full mode gives the same
    records' results."""
    k, r, e, p, _, seed = TUPLES[1]
    nb = 512
    c = case(k, r, e, p, TUPLES[1][4], seed, 64, cut=nb)
    work, rep = damaged(c)
    got, st, rec = run(eng, c, work, rep)
    check_full(c, work, got, st, rec, c.full)
    for plan in (1, 2, 3, 4, 5):
        with eng.knob("plan", plan):
            g2, s2, r2 = run(eng, c, work, rep)
        assert np.array_equal(g2, got) and np.array_equal(s2, st) and np.array_equal(r2, rec), plan
