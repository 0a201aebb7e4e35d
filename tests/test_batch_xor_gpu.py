"""XOR blocks through the batching adapter's gather path: connections with registered arenas, XOR jobs
mixed with RLC jobs in one batcher.  Every XOR symbol that lies in an arena is handed to the engine where it
lies, for its own length (fecgpu_xor_encode_rows_host / fecgpu_xor_decode_rows_host): nothing is staged,
the repair and the recovered symbol are written where they stay, and bytes, lengths, FPIDs, return values,
counters and completion order are those of the synchronous XOR operations."""
import numpy as np
import pytest

from oracle_py import DEC_RECOVERED, Oracle
from test_batch_gpu import Batch

pytestmark = pytest.mark.gpu

RLC_K, RLC_R = 8, 3


def _sources(rng, k, kind, max_symbol):
    """k source symbols: all max_symbol long, or ragged (1..1200 bytes, one of them 1200, one an odd tail)."""
    if kind == "equal":
        return [rng.integers(0, 256, max_symbol, dtype=np.uint8) for _ in range(k)]
    n = [int(x) for x in rng.integers(1, 1201, k)]
    n[int(rng.integers(0, k))] = int(rng.choice([1, 2, 3, 5, 1197, 1199]))
    n[int(rng.integers(0, k))] = 1200
    return [rng.integers(0, 256, x, dtype=np.uint8) for x in n]


@pytest.mark.parametrize("kind,max_symbol", [("equal", 1200), ("ragged", 1500)])
@pytest.mark.parametrize("batch_blocks", [5, 64])
def test_xor_generate_in_place(batch_blocks, kind, max_symbol):
    ncon = 4
    bt = Batch(batch_blocks, max_symbol=max_symbol, connections=ncon, conn_bytes=8 << 20)
    rng = np.random.default_rng(batch_blocks + max_symbol)
    o = Oracle()
    jobs, rows = [], 0
    for i in range(70):
        bt.use(i % ncon)
        fbn = int(rng.integers(0, 1 << 24))
        if i % 3 == 2:  # an RLC block between the XOR ones: its own job, the same batcher
            srcs = _sources(rng, RLC_K, kind, max_symbol)
            jobs.append((bt.generate(False, fbn, srcs, RLC_R, now=i), False, fbn, srcs))
            rows += RLC_K + RLC_R
        else:
            k = (4, 7, 1, 16)[i % 4]
            srcs = _sources(rng, k, kind, max_symbol)
            jobs.append((bt.generate(True, fbn, srcs, 1, now=i), True, fbn, srcs))
            rows += k + 1
    bt.L.mh_batch_drain()
    for t, xor, fbn, srcs in jobs:
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        ret, want = (0, [o.xor_encode_block(srcs)[1]]) if xor else o.rlc_encode_block(fbn, srcs, RLC_R)
        assert ret == 0
        maxl = max(len(s) for s in srcs)
        assert [len(x) for x in reps] == [maxl] * len(want)
        assert [x.tobytes() for x in reps] == [x.tobytes() for x in want], (xor, fbn)
        assert fps == [(fbn << 8) | x for x in range(len(want))]
    order = [bt.L.mh_batch_order(t) for t, *_ in jobs]
    assert sorted(order) == list(range(len(jobs)))
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == len(jobs)
    # before the XOR row forms every row of an XOR block was staged
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == rows, st
    bt.close()  # every symbol freed


def _xor_recover_jobs(rng, o, n, kind, max_symbol):
    out = []
    for i in range(n):
        k = (4, 7, 2, 16, 1)[i % 5]
        fbn = int(rng.integers(0, 1 << 24))
        full = _sources(rng, k, kind, max_symbol)
        rep = o.xor_encode_block(full)[1]
        miss = (0, k - 1, int(rng.integers(0, k)))[i % 3]
        srcs = [None if j == miss else full[j] for j in range(k)]
        st, want = o.xor_decode_block(srcs, [rep])
        assert st == DEC_RECOVERED and list(want) == [miss]
        out.append((fbn, k, miss, full, srcs, rep, want[miss]))
    return out


@pytest.mark.parametrize("kind,max_symbol", [("equal", 1200), ("ragged", 1500)])
@pytest.mark.parametrize("batch_blocks", [5, 64])
def test_xor_recover_in_place(batch_blocks, kind, max_symbol):
    ncon = 4
    bt = Batch(batch_blocks, max_symbol=max_symbol, connections=ncon, conn_bytes=8 << 20)
    rng = np.random.default_rng(100 + batch_blocks + max_symbol)
    o = Oracle()
    jobs, rows = [], 0
    for i, (fbn, k, miss, full, srcs, rep, want) in enumerate(_xor_recover_jobs(rng, o, 60, kind, max_symbol)):
        bt.use(i % ncon)
        jobs.append((bt.recover(True, fbn, srcs, [rep], [fbn << 8], now=i), fbn, k, miss, full, want))
        rows += (k - 1) + 1 + 1  # received sources, the repair, the symbol allocated for the missing source
        if i % 4 == 3:  # an RLC recover between them
            fb2 = int(rng.integers(0, 1 << 24))
            f2 = _sources(rng, RLC_K, kind, max_symbol)
            r2 = list(o.rlc_encode_block(fb2, f2, RLC_R)[1])
            s2 = [None if j == 5 else f2[j] for j in range(RLC_K)]
            jobs.append((bt.recover(False, fb2, s2, r2, [(fb2 << 8) | x for x in range(RLC_R)], now=i), fb2, RLC_K,
                         None, f2, o.rlc_decode_block(fb2, s2, r2)[1]))
            rows += (RLC_K - 1) + RLC_R + 1
    bt.L.mh_batch_drain()
    for t, fbn, k, miss, full, want in jobs:
        assert bt.status(t) == (0, 1), fbn  # ret 0: a symbol was inserted
        got, cur = bt.recovered(t)
        maxl = max(len(s) for s in full)
        if miss is None:  # the RLC block: its recovered source counts
            assert sorted(got) == sorted(want) == [5] and got[5].tobytes() == want[5].tobytes() and cur == RLC_K
            continue
        assert list(got) == [miss], fbn
        assert len(got[miss]) == maxl and got[miss].tobytes() == want.tobytes(), fbn
        orig = full[miss]
        assert got[miss][:len(orig)].tobytes() == orig.tobytes() and not got[miss][len(orig):].any()
        assert cur == k - 1  # the XOR operation does not count its recovered symbol (xor_fec_scheme.c:72)
        assert bt.last_fpids[miss] == (fbn << 8) | miss
    order = [bt.L.mh_batch_order(t) for t, *_ in jobs]
    assert sorted(order) == list(range(len(jobs)))
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == len(jobs)
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == rows, st
    bt.close()  # every symbol freed, the recovered ones included


@pytest.mark.parametrize("kind,max_symbol", [("equal", 1200), ("ragged", 1500)])
def test_xor_on_a_connection_without_an_arena(kind, max_symbol):
    """Blocks of a connection whose symbols lie in no registered arena, in the same jobs as blocks of one
    that has one: the same bytes, their rows staged (at their own length) and copied out."""
    bt = Batch(16, max_symbol=max_symbol, connections=2, conn_bytes=8 << 20)
    rng = np.random.default_rng(max_symbol)
    o = Oracle()
    gen, rec, in_place, staged = [], [], 0, 0
    for i in range(24):
        k = (4, 7)[i % 2]
        with_arena = i % 3 != 0
        bt.use(0 if with_arena else -1)
        fbn = int(rng.integers(0, 1 << 24))
        srcs = _sources(rng, k, kind, max_symbol)
        gen.append((bt.generate(True, fbn, srcs, 1, now=i), fbn, srcs))
        in_place += (k + 1) * with_arena
        staged += (k + 1) * (not with_arena)
    for i, (fbn, k, miss, full, srcs, rep, want) in enumerate(_xor_recover_jobs(rng, o, 24, kind, max_symbol)):
        with_arena = i % 3 != 1
        bt.use(1 if with_arena else -1)
        rec.append((bt.recover(True, fbn, srcs, [rep], [fbn << 8], now=100 + i), fbn, k, miss, want))
        in_place += (k + 1) * with_arena
        staged += k * (not with_arena)  # received sources and the repair; the recovered symbol is copied into
    bt.L.mh_batch_drain()
    for t, fbn, srcs in gen:
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        assert [x.tobytes() for x in reps] == [o.xor_encode_block(srcs)[1].tobytes()], fbn
        assert fps == [fbn << 8]
    for t, fbn, k, miss, want in rec:
        assert bt.status(t) == (0, 1)
        got, cur = bt.recovered(t)
        assert list(got) == [miss] and got[miss].tobytes() == want.tobytes(), fbn
        assert cur == k - 1 and bt.last_fpids[miss] == (fbn << 8) | miss
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == len(gen) + len(rec)
    assert st["rows_in_place"] == in_place and st["rows_staged"] == staged, (st, in_place, staged)
    bt.close()
