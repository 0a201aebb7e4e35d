"""Ragged blocks through the batching adapter's gather path: connections with registered arenas and a
stride (max_symbol 1500) longer than most symbols.  Every symbol that lies in an arena is handed to the
engine where it lies, for its own length (fecgpu_rlc_encode_rows_len_host /
fecgpu_rlc_decode_rows_len_host): nothing is staged, and repairs, recovered symbols, lengths, FPIDs and
completion order are the reference's."""
import numpy as np
import pytest

from golden_io import load, sha
from oracle_py import Oracle
from test_batch_gpu import Batch, _decode_jobs

pytestmark = pytest.mark.gpu

MAX_SYMBOL = 1500
K, R = 8, 3


def _lengths(rng, kind, k):
    """Symbol lengths of one block: ragged below 1200, another block length, or whole (the stride)."""
    if kind == "whole":
        return [MAX_SYMBOL] * k
    top = 1200 if kind == "ragged" else int(rng.integers(1, MAX_SYMBOL + 1))
    n = [int(x) for x in rng.integers(1, top + 1, k)]
    n[int(rng.integers(0, k))] = top  # the block's length
    if kind == "ragged":
        n[int(rng.integers(0, k))] = int(rng.choice([1, 2, 3, 5, 1197, 1199]))  # odd tails
        if max(n) != top:
            n[0] = top
    return n


def _blocks(rng, n, k):
    kinds = ["ragged", "other", "whole", "ragged", "ragged", "other"]
    out = []
    for b in range(n):
        lens = _lengths(rng, kinds[b % len(kinds)], k)
        out.append((int(rng.integers(0, 1 << 24)), [rng.integers(1, 256, x, dtype=np.uint8) for x in lens]))
    return out


@pytest.mark.parametrize("batch_blocks", [5, 64])
def test_ragged_generate_in_place(batch_blocks):
    ncon = 4
    bt = Batch(batch_blocks, max_symbol=MAX_SYMBOL, connections=ncon, conn_bytes=8 << 20)
    rng = np.random.default_rng(20261019 + batch_blocks)
    o = Oracle()
    blocks = _blocks(rng, 90, K)
    tickets = []
    for i, (fbn, srcs) in enumerate(blocks):
        bt.use(i % ncon)
        tickets.append(bt.generate(False, fbn, srcs, R, now=i))
    bt.L.mh_batch_drain()
    for t, (fbn, srcs) in zip(tickets, blocks):
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        ret, want = o.rlc_encode_block(fbn, srcs, R)
        assert ret == 0
        maxl = max(len(s) for s in srcs)
        assert [len(x) for x in reps] == [maxl] * R
        assert [x.tobytes() for x in reps] == [x.tobytes() for x in want], fbn
        assert fps == [(fbn << 8) | i for i in range(R)]
    order = [bt.L.mh_batch_order(t) for t in tickets]
    assert order == sorted(order) and min(order) >= 0
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == len(blocks)
    # on the code before the ragged entry points every row of a block shorter than the stride was staged
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == len(blocks) * (K + R), st
    bt.close()


@pytest.mark.parametrize("batch_blocks", [5, 64])
def test_ragged_recover_in_place(batch_blocks):
    ncon = 4
    bt = Batch(batch_blocks, max_symbol=MAX_SYMBOL, connections=ncon, conn_bytes=8 << 20)
    rng = np.random.default_rng(20261020 + batch_blocks)
    o = Oracle()
    jobs, handed = [], 0
    for i, (fbn, full) in enumerate(_blocks(rng, 90, K)):
        reps = list(o.rlc_encode_block(fbn, full, R)[1])
        e = int(rng.integers(1, R + 1))
        miss = set(int(x) for x in rng.choice(K, e, replace=False))
        if i % 7 == 3 and e < R:
            reps[int(rng.integers(1, R))] = None  # a repair that never arrived (the first one sets the length)
        srcs = [None if j in miss else full[j] for j in range(K)]
        st, want = o.rlc_decode_block(fbn, srcs, reps)
        bt.use(i % ncon)
        t = bt.recover(False, fbn, srcs, reps, [(fbn << 8) | x for x in range(R)], now=i)
        jobs.append((t, fbn, srcs, want, max(len(s) for s in full)))
        # received sources and repairs, and one symbol allocated for every missing source
        handed += K + sum(x is not None for x in reps)
    bt.L.mh_batch_drain()
    n_rec = 0
    for t, fbn, srcs, want, maxl in jobs:
        assert bt.status(t) == (0, 1)
        got, cur = bt.recovered(t)
        assert sorted(got) == sorted(want), fbn
        for j in got:
            assert len(got[j]) == maxl and got[j].tobytes() == want[j].tobytes(), (fbn, j)
            assert bt.last_fpids[j] == ((fbn << 8) + j) & 0xFFFFFFFF
        assert cur == sum(s is not None for s in srcs) + len(got)
        n_rec += len(got)
    assert n_rec > 100
    order = [bt.L.mh_batch_order(t) for t, *_ in jobs]
    assert order == sorted(order) and min(order) >= 0
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == len(jobs)
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == handed, st
    bt.close()


def test_ragged_fixtures_in_place():
    """The reference's own ragged cases (encode_cases.json "varlen", decode_cases.json "varlen_cases")
    with every symbol in a registered arena and a stride above their lengths: recorded bytes, lengths and
    FPIDs, nothing staged."""
    bt = Batch(3, max_symbol=MAX_SYMBOL, connections=2, conn_bytes=8 << 20)
    gen = []
    for i, case in enumerate(c for c in load("encode_cases.json")["varlen"] if c["scheme"] == "rlc" and c["ret"] == 0):
        srcs = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in case["src_hex"]]
        if max(len(s) for s in srcs) > MAX_SYMBOL:
            continue
        bt.use(i % 2)
        gen.append((bt.generate(False, case["fbn"], srcs, case["r"], now=i), case))
    varlen_tags = {c["tag"] for c in load("decode_cases.json")["varlen_cases"]}
    rec = []
    for i, (case, srcs, reps, fp) in enumerate(_decode_jobs()):
        if case["tag"] not in varlen_tags or case["scheme"] != "rlc":
            continue
        if max([len(x) for x in srcs + reps if x is not None] + [1]) > MAX_SYMBOL:
            continue
        bt.use(i % 2)
        rec.append((bt.recover(False, case["fbn"], srcs, reps, fp, now=100 + i), case, srcs))
    assert gen and rec
    bt.L.mh_batch_drain()
    for t, case in gen:
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        assert [x.tobytes().hex() for x in reps] == case["rep_hex"], case.get("tag")
        assert fps == case["repair_fpid_raw"]
    for t, case, srcs in rec:
        ret, calls = bt.status(t)
        assert calls == 1, case["tag"]
        got, cur = bt.recovered(t)
        if case["crashed"]:
            assert ret == 0 and got == {}
            continue
        assert ret == case["ret"], case["tag"]
        assert {str(j): sha(v.tobytes()) for j, v in sorted(got.items())} == case["recovered"], case["tag"]
        assert {str(j): len(v) for j, v in got.items()} == case["recovered_len"]
        assert cur == sum(s is not None for s in srcs) + len(got)
    st = bt.stats()
    assert st["engine_errors"] == 0
    assert st["rows_staged"] == 0 and st["rows_in_place"] > 0, st
    bt.close()


def test_ragged_generate_arena_full_part_way_through_a_block():
    """The arena fills part way through a ragged block's allocations: the rows in it are coded in place
    and keep their bytes, the rest are staged at their own length and copied out."""
    # 13 slots: the first block's 4 sources (8 slots), repairs 0-1 (4 slots) and repair 2's struct;
    # repair 2's data and repair 3 come from the heap, as do the later blocks
    bt = Batch(4, max_symbol=MAX_SYMBOL, arena=True, arena_bytes=13 * 2112)
    rng = np.random.default_rng(12)
    o = Oracle()
    blocks = [(int(rng.integers(0, 1 << 24)), [rng.integers(1, 256, n, dtype=np.uint8) for n in (1200, 37, 1199, 640)])
              for _ in range(3)]
    tickets = [bt.generate(False, fbn, srcs, 4, now=i) for i, (fbn, srcs) in enumerate(blocks)]
    bt.L.mh_batch_drain()
    for t, (fbn, srcs) in zip(tickets, blocks):
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        assert [x.tobytes() for x in reps] == [x.tobytes() for x in o.rlc_encode_block(fbn, srcs, 4)[1]], fbn
        assert fps == [(fbn << 8) | i for i in range(4)]
    st = bt.stats()
    assert st["engine_errors"] == 0
    assert st["rows_in_place"] == 4 + 2 and st["rows_staged"] == 3 * 8 - 6, st
    bt.close()


def test_ragged_recover_arena_full_part_way_through_a_block():
    """Recover likewise: the first block's received symbols (12 slots) and its first recovered symbol (2
    slots) lie in the arena, its second recovered symbol's data and everything after come from the heap."""
    k, r = 6, 3
    bt = Batch(4, max_symbol=MAX_SYMBOL, arena=True, arena_bytes=15 * 2112)
    rng = np.random.default_rng(18)
    o = Oracle()
    jobs = []
    for b in range(3):
        fbn = int(rng.integers(0, 1 << 24))
        full = [rng.integers(1, 256, n, dtype=np.uint8) for n in (900, 1200, 3, 1199, 1200, 77)]
        reps = o.rlc_encode_block(fbn, full, r)[1]
        miss = {1, 3, 4}
        srcs = [None if j in miss else full[j] for j in range(k)]
        st, want = o.rlc_decode_block(fbn, srcs, list(reps))
        assert sorted(want) == sorted(miss)
        jobs.append((bt.recover(False, fbn, srcs, list(reps), [(fbn << 8) | i for i in range(r)], now=b), fbn, want))
    bt.L.mh_batch_drain()
    for t, fbn, want in jobs:
        assert bt.status(t) == (0, 1)
        got, cur = bt.recovered(t)
        assert sorted(got) == sorted(want), fbn
        for j in got:
            assert len(got[j]) == 1200 and got[j].tobytes() == want[j].tobytes(), (fbn, j)
        assert cur == k
    st = bt.stats()
    assert st["engine_errors"] == 0
    assert st["rows_in_place"] == 6 + 1 and st["rows_staged"] > 0, st
    bt.close()
