"""Full-rank RLC recovery where the hooks run: the resident block service (fecgpu_block_svc_rlc_decode_full,
the re-plan inside the worker) and the fec_recover protocol operation under pquic_fec_set_recover_mode(1),
driven through the picoquic stand-in exactly as the frameworks call it.  Patterns and verdicts come from
decode_full_cases.py (CPU only); ground truth for bytes is the original sources."""
import ctypes as C
import os

import numpy as np
import pytest

from decode_full_cases import RECOVERED, REF_UB, SINGULAR, TUPLES, case, damaged, gf, gf_rank, rows_for
from oracle_py import Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
DEV = "cuda:0"


def _sets():
    """(case, block indices) of the blocks the hooks are driven with: B's blocks solvable only through a later
    repair; A's blocks reference mode gives up on, its singular blocks and four it recovers."""
    a = case(*TUPLES[0], 1200)
    b = case(*TUPLES[1], 64, cut=512)
    later = np.nonzero(b.full & ~b.first)[0]
    give_up = np.nonzero((a.ref_st == REF_UB) & a.full)[0]
    singular = np.nonzero(~a.full)[0]
    ref_ok = np.nonzero(a.ref_st == RECOVERED)[0][:4]
    assert (later.size, give_up.size, singular.size, ref_ok.size) == (3, 29, 10, 4)
    assert (b.ref_st[later] == REF_UB).all()
    return (b, later), (a, np.concatenate([give_up, singular, ref_ok])), give_up, singular


def to_dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pinned(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    return t, t.numpy()


def seeds_of(idx, r):
    return (idx.astype(np.uint32)[:, None] << 8) | np.arange(r, dtype=np.uint32)[None, :]


# ------------------------------------------------------------------------------------------ block service
@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from pquic_amd import load_library
    return load_library()


@pytest.fixture(scope="module")
def svc(lib):
    v = lib.fecgpu_block_svc_create(0)
    assert v
    assert lib.fecgpu_block_svc_set_deadline(v, 1_000_000) == 0  # never withdrawn because a box was slow
    yield v
    lib.fecgpu_block_svc_destroy(v)


def test_block_service_full(lib, svc):
    from pquic_amd import Engine
    eng = Engine(0)
    (cb, ib), (ca, ia), give_up, _ = _sets()
    calls, checks = [], []
    for c, idx in ((cb, ib), (ca, ia)):
        k, r, L, n = c.k, c.r, c.L, idx.size
        work_all, rep_all = damaged(c)
        work, rep = work_all[idx], rep_all[idx]
        seeds = seeds_of(idx, r)
        # what fecgpu_rlc_decode_full gives on the same blocks
        w = to_dev(work)
        st_d = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        rec_d = torch.full((n, 2), -1, dtype=torch.int64, device=DEV)
        eng.rlc_decode_full(w, to_dev(rep), to_dev(c.sp[idx]), to_dev(c.rp[idx]), st_d, rec_d, k, r, L, nblocks=n,
                            rep_seed=to_dev(seeds.reshape(-1)))
        torch.cuda.synchronize()
        exp_st = np.where(c.full[idx], RECOVERED, SINGULAR).astype(np.uint8)
        assert np.array_equal(st_d.cpu().numpy(), exp_st)
        assert np.array_equal(w.cpu().numpy()[c.full[idx]], c.src[idx][c.full[idx]])
        # page-locked buffers for every call, made before the series so that the series is only calls
        tw, hw = pinned(work)
        trp, _ = pinned(rep)
        tse, _ = pinned(seeds)
        tsp, _ = pinned(c.sp[idx].view(np.int64))
        trm, _ = pinned(c.rp[idx].view(np.int64))
        tst, hst = pinned(np.full((n, 16), 0xEE, np.uint8))
        trec, hrec = pinned(np.full((n, 2), -1, np.int64))
        for x in range(n):
            calls.append((tw[x].data_ptr(), trp[x].data_ptr(), tw[x].data_ptr(), k, r, L, tse[x].data_ptr(),
                          tsp[x].data_ptr(), trm[x].data_ptr(), tst[x].data_ptr(), trec[x].data_ptr()))
        checks.append((hw, hst, hrec, w.cpu().numpy(), st_d.cpu().numpy(), rec_d.cpu().numpy(),
                       (tw, trp, tse, tsp, trm, tst, trec)))
    # a reference-mode request between two full ones on a block reference mode gives up on: its own buffers
    c, x = ca, int(give_up[0])
    work_all, rep_all = damaged(c)
    tw2, hw2 = pinned(work_all[x:x + 1])
    trp2, _ = pinned(rep_all[x:x + 1])
    tse2, _ = pinned(seeds_of(np.array([x]), c.r))
    tsp2, _ = pinned(c.sp[x:x + 1].view(np.int64))
    trm2, _ = pinned(c.rp[x:x + 1].view(np.int64))
    tst2, hst2 = pinned(np.full(16, 0xEE, np.uint8))
    trec2, _ = pinned(np.full((1, 2), -1, np.int64))
    ref_call = (tw2.data_ptr(), trp2.data_ptr(), tw2.data_ptr(), c.k, c.r, c.L, tse2.data_ptr(), tsp2.data_ptr(),
                trm2.data_ptr(), tst2.data_ptr(), trec2.data_ptr())
    full, seeded = lib.fecgpu_block_svc_rlc_decode_full, lib.fecgpu_block_svc_rlc_decode_seeded
    n0 = lib.fecgpu_block_svc_launches(svc)
    rcs = [full(svc, *a) for a in calls[:4]]
    rc_ref = seeded(svc, *ref_call)
    rcs += [full(svc, *a) for a in calls[4:]]
    n1 = lib.fecgpu_block_svc_launches(svc)
    assert rcs == [0] * len(calls) and rc_ref == 0, lib.fecgpu_last_error()
    assert n1 - n0 <= 1  # every request was served by the resident worker
    assert hst2[0] == REF_UB and np.array_equal(hw2, work_all[x:x + 1])  # the mode is the request's own
    for hw, hst, hrec, w_d, st_d, rec_d, _ in checks:
        assert np.array_equal(hst[:, 0], st_d)
        assert np.array_equal(hrec, rec_d)
        assert np.array_equal(hw, w_d)


# ------------------------------------------------------------------------------------------ protocol operations
@pytest.fixture(scope="module")
def host():
    from test_protoops_gpu import Host
    return Host()


@pytest.fixture()
def fec(host):
    """libpquic_fec.so by the path libminihost.so links it by (one copy in the process); the mode goes back to
    0 whatever happens."""
    L = C.CDLL(LIB)
    L.pquic_fec_set_recover_mode.argtypes = [C.c_int]
    L.pquic_fec_singular_blocks.restype = C.c_uint64
    try:
        yield L
    finally:
        L.pquic_fec_set_recover_mode(0)


def ref_ub_blocks(host):
    st = np.zeros(5, np.uint64)
    host.lib.mh_protoop_stats(st.ctypes.data_as(C.POINTER(C.c_uint64)))
    return int(st[3])


def _hook_blocks():
    """Every block of _sets() as the framework hands it over: sources of varying length (one as long as the
    block, some all zero), the repairs of exactly those sources, fbn = the block's index in its case."""
    o = Oracle()
    rng = np.random.default_rng(2026)
    (cb, ib), (ca, ia), _, _ = _sets()
    out = []
    for c, idx in ((cb, ib), (ca, ia)):
        for b in idx:
            b = int(b)
            lens = rng.integers(1, c.L + 1, c.k)
            lens[rng.integers(0, c.k)] = c.L
            full_src = [c.src[b, j, :lens[j]].copy() for j in range(c.k)]
            if b % 3 == 0 and c.ref_st[b] == REF_UB:  # (reference mode's zero rule may hide other symbols)
                full_src[int(c.miss[b][0])][:] = 0  # a missing all-zero source: recovered as zeros, not inserted
            ret, reps = o.rlc_encode_block(b, full_src, c.r)
            assert ret == 0 and all(len(x) == c.L for x in reps)
            srcs = [None if j in set(c.miss[b].tolist()) else full_src[j] for j in range(c.k)]
            rin = [reps[i] if i in set(c.present[b].tolist()) else None for i in range(c.r)]
            want = {}
            for j in c.miss[b]:
                row = np.zeros(c.L, np.uint8)
                row[:lens[j]] = full_src[j]
                if row.any():
                    want[int(j)] = row
            out.append(dict(fbn=b, srcs=srcs, reps=rin, fpids=[(b << 8) | i for i in range(c.r)], want=want,
                            full=bool(c.full[b]), ref_st=int(c.ref_st[b]), maxl=c.L))
    return out


def _check_recovered(host, blk, ret, rec, cur):
    assert ret == 0
    assert sorted(rec) == sorted(blk["want"]), blk["fbn"]
    for j, row in blk["want"].items():
        assert len(rec[j]) == blk["maxl"] and np.array_equal(rec[j], row), (blk["fbn"], j)
        assert host.last_fpids[j] == (blk["fbn"] << 8) + j
    assert cur == sum(s is not None for s in blk["srcs"]) + len(rec)


def test_protoops_recover_modes(host, fec):
    blocks = _hook_blocks()
    n_singular = sum(not b["full"] for b in blocks)
    n_ref_ub = sum(b["ref_st"] == REF_UB for b in blocks)
    assert n_singular == 10 and n_ref_ub == 3 + 29 + 10
    live0 = host.lib.mh_live_allocations()
    # mode 0: what these blocks give today
    assert fec.pquic_fec_get_recover_mode() == 0
    ub0, sing0 = ref_ub_blocks(host), fec.pquic_fec_singular_blocks()
    given_up = None
    for blk in blocks:
        ret, rec, cur = host.recover(False, blk["fbn"], blk["srcs"], blk["reps"], blk["fpids"])
        if blk["ref_st"] == REF_UB:
            assert ret == 0 and rec == {} and cur == sum(s is not None for s in blk["srcs"]), blk["fbn"]
            given_up = (ret, rec, cur - sum(s is not None for s in blk["srcs"]))
        else:
            _check_recovered(host, blk, ret, rec, cur)
    assert ref_ub_blocks(host) == ub0 + n_ref_ub and fec.pquic_fec_singular_blocks() == sing0
    # mode 1
    assert fec.pquic_fec_set_recover_mode(1) == 0
    ub1 = ref_ub_blocks(host)
    for blk in blocks:
        ret, rec, cur = host.recover(False, blk["fbn"], blk["srcs"], blk["reps"], blk["fpids"])
        if blk["full"]:
            _check_recovered(host, blk, ret, rec, cur)
        else:  # what a block reference mode gives up on returns in mode 0; nothing inserted
            assert (ret, rec, cur - sum(s is not None for s in blk["srcs"])) == given_up, blk["fbn"]
    assert fec.pquic_fec_singular_blocks() == sing0 + n_singular
    assert ref_ub_blocks(host) == ub1
    assert host.lib.mh_live_allocations() == live0
    # and back
    assert fec.pquic_fec_set_recover_mode(0) == 0
    blk = next(b for b in blocks if b["full"] and b["ref_st"] == REF_UB)
    ret, rec, _ = host.recover(False, blk["fbn"], blk["srcs"], blk["reps"], blk["fpids"])
    assert ret == 0 and rec == {}


def test_protoops_window_block_through_a_later_repair(host, fec):
    """A sliding-window block -- numbered by its window start, its repairs carrying block number 0 -- whose
    first n received repairs are dependent on the missing columns while a later one is not."""
    k, r, e, p, nb, seed = TUPLES[1]
    c = case(k, r, e, p, nb, seed, 64, cut=512)
    rows = rows_for(lambda b, i: i, k, c.miss, c.present)
    full, first = gf_rank(rows) == e, gf_rank(rows[:, :e]) == e
    pick = np.nonzero(full & ~first)[0]
    assert pick.size > 0
    b = int(pick[0])
    o = Oracle()
    mul, _ = gf()
    L, start = 64, 0x1234
    rep = np.zeros((r, L), np.uint8)
    for i in range(r):
        coef = o.coefs(i, k)  # seed (0 << 8) | i
        for j in range(k):
            rep[i] ^= mul[coef[j]][c.src[b, j]]
    miss, present = set(c.miss[b].tolist()), set(c.present[b].tolist())
    srcs = [None if j in miss else c.src[b, j].copy() for j in range(k)]
    reps = [rep[i].copy() if i in present else None for i in range(r)]
    fpids = list(range(r))
    ret, rec, _ = host.recover(False, start, srcs, reps, fpids)  # mode 0: given up
    assert ret == 0 and rec == {}
    assert fec.pquic_fec_set_recover_mode(1) == 0
    ret, rec, cur = host.recover(False, start, srcs, reps, fpids)
    assert ret == 0 and sorted(rec) == sorted(miss)
    for j in miss:
        assert np.array_equal(rec[j], c.src[b, j]) and host.last_fpids[j] == (start << 8) + j
    assert cur == k
