"""Window jobs through the batching adapter over a registered arena: the streams of
test_batch_window_generate_sliding (lengths 1200, 1-1500 and 1-39, steps 1-7, a gap, a repeated window, k
changing mid-stream), submitted interleaved.  With the window row form in the engine
(fecgpu_rlc_window_encode_rows_host) the jobs gather: every stream symbol and every repair in the arena is
handed over where it lies (rows_in_place counts each stream row once and each repair row once, none is
staged), and repairs and FPIDs are the oracle's block-number-0 encode of the window's symbols."""
import numpy as np
import pytest

from oracle_py import Oracle
from test_batch_gpu import Batch

pytestmark = pytest.mark.gpu


def _streams(rng):
    """(symbols, [(start, k)], r) per connection"""
    out = []
    lens_kinds = [lambda: 1200, lambda: 1200, lambda: int(rng.integers(1, 1501)), lambda: int(rng.integers(1, 40))]
    for c in range(8):
        n = 160
        syms = [rng.integers(0, 256, lens_kinds[c % 4](), dtype=np.uint8) for _ in range(n)]
        step = [1, 2, 3, 7, 1, 5, 2, 4][c]
        k = [30, 20, 30, 12, 1, 30, 16, 25][c]
        r = [4, 4, 8, 2, 1, 6, 4, 5][c]
        wins = [(s0, k) for s0 in range(0, n - k - 40, step)]
        wins.append((wins[-1][0] + k + 3, k))  # a gap: nothing shared with the window before
        wins.append(wins[-1])                  # the same window again
        k2 = max(1, k - 3)                      # window length changes (another queue)
        wins += [(s0, k2) for s0 in range(wins[-1][0] + 1, n - k2, step)]
        out.append((syms, wins, r))
    return out


_ref = {}


def _want(o, streams, c, s0, k, r):
    """The oracle's repairs of one window, computed once."""
    key = (c, s0, k)
    if key not in _ref:
        ret, reps = o.rlc_encode_block(0, streams[c][0][s0: s0 + k], r)
        assert ret == 0
        _ref[key] = [x.tobytes() for x in reps]
    return _ref[key]


def _run(bt, streams):
    sids = [bt.open_stream(syms) for syms, _, _ in streams]
    pending = [list(w) for _, w, _ in streams]
    tickets = []
    now = 0
    while any(pending):
        for c, (syms, _, r) in enumerate(streams):
            if pending[c]:
                s0, k = pending[c].pop(0)
                tickets.append((c, s0, k, r, bt.generate_window(sids[c], s0, k, r, now=now)))
                now += 1
                if now % 97 == 0:
                    bt.L.mh_batch_poll(now)
    bt.L.mh_batch_drain()
    return tickets


def _check(bt, o, streams, tickets):
    for c, s0, k, r, t in tickets:
        assert bt.status(t) == (0, 1)
        reps, fps = bt.repairs(t)
        assert [x.tobytes() for x in reps] == _want(o, streams, c, s0, k, r), (c, s0, k)
        assert fps == list(range(r))
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["windows"] == len(tickets)
    return st


@pytest.fixture(scope="module")
def streams():
    _ref.clear()
    return _streams(np.random.default_rng(20261020))


@pytest.mark.parametrize("batch_blocks", [7, 64])
def test_window_jobs_run_in_place(streams, batch_blocks):
    bt = Batch(batch_blocks, max_symbol=1500, arena=True)
    o = Oracle()
    tickets = _run(bt, streams)
    st = _check(bt, o, streams, tickets)
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == st["window_rows"] + sum(r for _, _, _, r, _ in tickets), st
    bt.close()


def test_window_jobs_with_part_of_the_symbols_outside_the_arena(streams):
    """An arena of 1500 slots: the first 750 stream symbols (a struct and a data slot each) lie in it, the
    others and every repair come from the heap and go through staging rows."""
    bt = Batch(64, max_symbol=1500, arena=True, arena_bytes=1500 * 2112)
    o = Oracle()
    tickets = _run(bt, streams)
    st = _check(bt, o, streams, tickets)
    assert st["rows_staged"] > 0 and st["rows_in_place"] > 0, st
    assert st["rows_staged"] + st["rows_in_place"] == st["window_rows"] + sum(r for _, _, _, r, _ in tickets), st
    bt.close()
