"""Full-rank RLC recovery through the batching adapter: a batcher created under PQUIC_FEC_BATCH_FULL_RANK=1
runs its RLC recover jobs through the engine's *_full host forms -- in place with a registered arena (whole
blocks and ragged ones) and staged without one -- and completes every block the received repairs determine,
with the reference's FPIDs, lengths, completion order and allocation behaviour.  Patterns and verdicts come
from decode_full_cases.py (CPU only); ground truth for bytes is the original sources."""
import os

import numpy as np
import pytest

from decode_full_cases import RECOVERED, REF_UB, TUPLES, case
from oracle_py import Oracle
from test_batch_gpu import Batch

pytestmark = pytest.mark.gpu

ENV = "PQUIC_FEC_BATCH_FULL_RANK"
L = 64


def open_batch(full_rank, **kw):
    """A batcher made with the variable set to 1 (or unset), and the variable as it was afterwards."""
    old = os.environ.pop(ENV, None)
    try:
        if full_rank:
            os.environ[ENV] = "1"
        return Batch(128, max_symbol=L, **kw)
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def _blocks(ragged):
    """128 blocks of case B -- those reference mode gives up on though the repairs determine them (the ones
    solvable only through a later repair among them), the rest blocks it recovers -- then A's singular
    blocks, which form a second queue (r = 4).  Every block as (fbn, srcs, reps, fpids, want, ref_st, full)."""
    cb = case(*TUPLES[1], L, cut=512)
    ca = case(*TUPLES[0], L)
    give_up = np.nonzero((cb.ref_st == REF_UB) & cb.full)[0]
    later = np.nonzero(cb.full & ~cb.first)[0]
    assert give_up.size == 7 and later.size == 3 and (~cb.full).sum() == 0
    special = np.union1d(give_up, later)
    ref_ok = np.nonzero(cb.ref_st == RECOVERED)[0][:128 - special.size]
    singular = np.nonzero(~ca.full)[0]
    assert singular.size == 10
    o = Oracle()
    rng = np.random.default_rng(77 + ragged)
    out = []
    # the special blocks spread through the batch, not at its head
    order_b = np.concatenate([ref_ok[:40], special, ref_ok[40:]])
    for c, idx in ((cb, order_b), (ca, singular)):
        for b in idx:
            b = int(b)
            lens = np.full(c.k, L)
            if ragged:
                lens = rng.integers(1, L + 1, c.k)
                lens[rng.integers(0, c.k)] = L
            full_src = [c.src[b, j, :lens[j]].copy() for j in range(c.k)]
            for s in full_src:
                s[s == 0] = 1  # no all-zero source: reference mode's zero rule stays out of the way
            ret, reps = o.rlc_encode_block(b, full_src, c.r)
            assert ret == 0 and all(len(x) == L for x in reps)
            miss, present = set(c.miss[b].tolist()), set(c.present[b].tolist())
            srcs = [None if j in miss else full_src[j] for j in range(c.k)]
            rin = [reps[i] if i in present else None for i in range(c.r)]
            want = {}
            for j in miss:
                want[j] = np.zeros(L, np.uint8)
                want[j][:lens[j]] = full_src[j]
            out.append(dict(fbn=b, srcs=srcs, reps=rin, fpids=[(b << 8) | i for i in range(c.r)], want=want,
                            ref_st=int(c.ref_st[b]), full=bool(c.full[b])))
    assert len(out) == 138
    return out


def _run(bt, blocks, full_rank):
    live0 = bt.L.mh_live_allocations()
    tickets = [bt.recover(False, b["fbn"], b["srcs"], b["reps"], b["fpids"], now=i) for i, b in enumerate(blocks)]
    bt.L.mh_batch_drain()
    held = 0
    n_solved = 0
    for t, b in zip(tickets, blocks):
        assert bt.status(t) == (0, 1), b["fbn"]  # one completion per block
        got, cur = bt.recovered(t)
        present = sum(s is not None for s in b["srcs"])
        solved = b["full"] if full_rank else b["ref_st"] == RECOVERED
        if solved:
            assert sorted(got) == sorted(b["want"]), b["fbn"]
            for j, row in b["want"].items():
                assert len(got[j]) == L and np.array_equal(got[j], row), (b["fbn"], j)
                assert bt.last_fpids[j] == (b["fbn"] << 8) + j
        else:
            assert got == {}, b["fbn"]
        assert cur == present + len(got)
        held += present + sum(x is not None for x in b["reps"]) + len(got)
        n_solved += solved
    order = [bt.L.mh_batch_order(t) for t in tickets]
    assert order == sorted(order) and min(order) >= 0  # completions in submission order
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == len(blocks) and st["batches"] == 2
    # every symbol still alive belongs to a block (struct + data): each unrecovered pre-allocation was freed
    assert bt.L.mh_live_allocations() == live0 + 2 * held
    return n_solved, st


@pytest.mark.parametrize("cfg", ["arena_equal", "arena_ragged", "staged"])
def test_batch_full_rank(cfg):
    blocks = _blocks(cfg == "arena_ragged")
    n_full = sum(b["full"] for b in blocks)
    n_ref = sum(b["ref_st"] == RECOVERED for b in blocks)
    assert n_full == 128 and n_ref == 128 - 7  # the later-repair blocks are among the seven given up on
    import ctypes as C
    fec = C.CDLL(os.path.join(os.path.dirname(__file__), "..", "pquic_amd", "lib", "libpquic_fec.so"))
    fec.pquic_fec_singular_blocks.restype = C.c_uint64
    sing0 = fec.pquic_fec_singular_blocks()
    bt = open_batch(True, arena=cfg != "staged", arena_bytes=64 << 20)
    live_arena = bt.L.mh_arena_live(-1)
    n_solved, st = _run(bt, blocks, True)
    assert n_solved == n_full
    assert fec.pquic_fec_singular_blocks() == sing0 + 10
    if cfg == "staged":
        assert st["rows_in_place"] == 0
    else:
        assert st["rows_staged"] == 0 and st["rows_in_place"] > 0, st
    bt.close()  # (asserts that nothing leaked)
    if cfg != "staged":
        assert bt.L.mh_arena_live(-1) == live_arena  # arena live count back at its baseline
    # the variable unset: what the same batch gives today
    bt = open_batch(False, arena=cfg != "staged", arena_bytes=64 << 20)
    n_solved, _ = _run(bt, blocks, False)
    assert n_solved == n_ref
    assert fec.pquic_fec_singular_blocks() == sing0 + 10
    bt.close()
