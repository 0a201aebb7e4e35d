"""A ragged generate-then-recover round through the batching adapter over registered arenas: the repairs the
batcher generates are erased against and fed back to its recover, at k16 r4 and k32 r8, 64 blocks per batch.
With the one-pass row forms in the engine (fecgpu_rlc_*_rows_fused_host) the jobs run through them: every
row is handed over where it lies (rows_in_place counts every row, none is staged), and repairs and recovered
symbols are the oracle's."""
import numpy as np
import pytest

from oracle_py import Oracle
from test_batch_gpu import Batch
from test_batch_ragged_gpu import MAX_SYMBOL, _lengths

pytestmark = pytest.mark.gpu

NBLOCKS = 64


@pytest.mark.parametrize("k,r", [(16, 4), (32, 8)])
def test_ragged_round_in_place(k, r):
    ncon = 4
    rng = np.random.default_rng([20261020, k, r])
    o = Oracle()
    blocks = []
    for _ in range(NBLOCKS):
        lens = _lengths(rng, "ragged", k)
        blocks.append((int(rng.integers(0, 1 << 24)), [rng.integers(1, 256, x, dtype=np.uint8) for x in lens]))
    # generate
    bt = Batch(NBLOCKS, max_symbol=MAX_SYMBOL, connections=ncon, conn_bytes=16 << 20)
    tickets = []
    for i, (fbn, srcs) in enumerate(blocks):
        bt.use(i % ncon)
        tickets.append(bt.generate(False, fbn, srcs, r, now=i))
    bt.L.mh_batch_drain()
    repairs = []
    for t, (fbn, srcs) in zip(tickets, blocks):
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        ret, want = o.rlc_encode_block(fbn, srcs, r)
        assert ret == 0
        assert [x.tobytes() for x in reps] == [x.tobytes() for x in want], fbn
        assert fps == [(fbn << 8) | i for i in range(r)]
        repairs.append([np.array(x, np.uint8) for x in reps])
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == NBLOCKS
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == NBLOCKS * (k + r), st
    bt.close()
    # recover from the batcher's own repairs
    bt = Batch(NBLOCKS, max_symbol=MAX_SYMBOL, connections=ncon, conn_bytes=16 << 20)
    jobs, handed = [], 0
    for i, ((fbn, full), reps) in enumerate(zip(blocks, repairs)):
        e = int(rng.integers(1, r + 1))
        miss = set(int(x) for x in rng.choice(k, e, replace=False))
        reps = list(reps)
        if i % 5 == 2 and e < r:
            reps[int(rng.integers(1, r))] = None  # a repair that never arrived (the first one sets the length)
        srcs = [None if j in miss else full[j] for j in range(k)]
        status, want = o.rlc_decode_block(fbn, srcs, reps)
        bt.use(i % ncon)
        t = bt.recover(False, fbn, srcs, reps, [(fbn << 8) | x for x in range(r)], now=i)
        jobs.append((t, fbn, full, srcs, want))
        handed += k + sum(x is not None for x in reps)
    bt.L.mh_batch_drain()
    n_rec = 0
    for t, fbn, full, srcs, want in jobs:
        assert bt.status(t) == (0, 1)
        got, cur = bt.recovered(t)
        assert sorted(got) == sorted(want), fbn
        maxl = max(len(s) for s in full)
        for j in got:
            assert len(got[j]) == maxl and got[j].tobytes() == want[j].tobytes(), (fbn, j)
            assert got[j][:len(full[j])].tobytes() == full[j].tobytes() and not got[j][len(full[j]):].any()
        assert cur == sum(s is not None for s in srcs) + len(got)
        n_rec += len(got)
    assert n_rec >= NBLOCKS  # most blocks recover: a round that recovered nothing would check nothing
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["completed"] == NBLOCKS
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == handed, st
    bt.close()
