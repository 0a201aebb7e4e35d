"""Mixed window jobs through the batching adapter (PQUIC_FEC_BATCH_WINDOW_MIXED=1 at creation,
pquic_fec_batch_set_window_mixed): a window sender protects whatever is in flight, so a connection's window
length changes with every send.  Eight connections, each length a seeded random walk in 1..30 with steps
-3..+3, r per connection 1, 4 or 8 (min(r, length) for a short window, as the sender sets it), symbol lengths
1200, 1..1500 and 1..39, submitted interleaved with polls.  Windows of several lengths share a job keyed by
(kclass, r), kclass the smallest of 16, 32, 64, 128 that holds the window; every ticket's repairs and FPIDs are
the oracle's block-number-0 encode of the window's own symbols."""
import os

import numpy as np
import pytest

from oracle_py import Oracle
from test_batch_gpu import Batch

pytestmark = pytest.mark.gpu

ENV = "PQUIC_FEC_BATCH_WINDOW_MIXED"


def open_batch(mixed, *a, **kw):
    """A batcher made with the variable set to 1 (or unset), and the variable as it was afterwards."""
    old = os.environ.pop(ENV, None)
    try:
        if mixed:
            os.environ[ENV] = "1"
        return Batch(*a, **kw)
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def _streams(rng, top=1500):
    """(symbols, [(start, length, r)]) per connection: the window's end advances 1..3 symbols per send, its
    length walks, and the sender asks for min(r, length) repairs.  top: the longest symbol."""
    out = []
    full = min(top, 1200)
    lens_kinds = [lambda: full, lambda: full, lambda: int(rng.integers(1, top + 1)), lambda: int(rng.integers(1, 40))]
    for c in range(8):
        n = 160
        syms = [rng.integers(0, 256, lens_kinds[c % 4](), dtype=np.uint8) for _ in range(n)]
        r = [4, 8, 1, 4, 8, 4, 1, 8][c]
        length, end, wins = int(rng.integers(1, 31)), 30, []
        while end <= n:
            wins.append((end - length, length, min(r, length)))
            length = int(np.clip(length + rng.integers(-3, 4), 1, 30))
            end += int(rng.integers(1, 4))
        if c == 3:
            wins.append(wins[-1])  # the same window again
        out.append((syms, wins))
    return out


_ref = {}


def _want(o, streams, c, s0, k, r):
    """The oracle's repairs of one window, computed once."""
    key = (id(streams), c, s0, k, r)
    if key not in _ref:
        ret, reps = o.rlc_encode_block(0, streams[c][0][s0: s0 + k], r)
        assert ret == 0
        _ref[key] = [x.tobytes() for x in reps]
    return _ref[key]


def _run(bt, streams, poll=True):
    sids = [bt.open_stream(syms) for syms, _ in streams]
    pending = [list(w) for _, w in streams]
    tickets = []
    now = 0
    while any(pending):
        for c in range(len(streams)):
            if pending[c]:
                s0, k, r = pending[c].pop(0)
                tickets.append((c, s0, k, r, bt.generate_window(sids[c], s0, k, r, now=now)))
                now += 1
                if poll and now % 97 == 0:
                    bt.L.mh_batch_poll(now)
    bt.L.mh_batch_drain()
    return tickets


def _check(bt, o, streams, tickets):
    got = []
    for c, s0, k, r, t in tickets:
        assert bt.status(t) == (0, 1)  # done exactly once
        reps, fps = bt.repairs(t)
        assert [x.tobytes() for x in reps] == _want(o, streams, c, s0, k, r), (c, s0, k, r)
        assert fps == list(range(r))
        got.append(reps)
    order = [bt.L.mh_batch_order(t) for _, _, _, _, t in tickets]
    st = bt.stats()
    assert st["engine_errors"] == 0 and st["windows"] == len(tickets) == st["completed"]
    return st, got, order


def _kclass(k):
    return 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128


@pytest.fixture(scope="module")
def streams():
    _ref.clear()
    s = _streams(np.random.default_rng(20261021))
    lens = {k for _, w in s for _, k, _ in w}
    assert 1 in lens and 30 in lens and len(lens) >= 25, "the walks visit nearly every length"
    assert any(r < rr for (_, w), rr in zip(s, [4, 8, 1, 4, 8, 4, 1, 8]) for _, _, r in w), "a window shorter than r"
    return s


@pytest.fixture(scope="module")
def small_streams():
    """walks of the same kind over symbols of at most 64 bytes: jobs of a whole run's windows stay small"""
    return _streams(np.random.default_rng(20261021), top=64)


@pytest.mark.parametrize("batch_blocks", [7, 64])
def test_mixed_window_jobs_run_in_place(streams, batch_blocks):
    bt = open_batch(True, batch_blocks, max_symbol=1500, arena=True)
    o = Oracle()
    tickets = _run(bt, streams)
    st, _, _ = _check(bt, o, streams, tickets)
    assert st["rows_staged"] == 0, st
    assert st["rows_in_place"] == st["window_rows"] + sum(r for _, _, _, r, _ in tickets), st
    bt.close()


def test_one_job_per_class_and_fewer_batches_than_a_queue_per_length(small_streams):
    """batch_blocks above the window count, no deadline, one drain: a batch per distinct (kclass, r); the same
    streams with the variable unset take a batch per distinct (k, r) or more, and give the same bytes.  (Symbols
    of at most 64 bytes: the unset run opens some fifty queues, each with page-locked rows for every window.)"""
    streams = small_streams
    o = Oracle()
    nwin = sum(len(w) for _, w in streams)
    bt = open_batch(True, nwin + 1, max_delay_us=10 ** 9, max_symbol=64, arena=True)
    tickets = _run(bt, streams, poll=False)
    st, mixed, order = _check(bt, o, streams, tickets)
    pairs = {(_kclass(k), r) for _, _, k, r, _ in tickets}
    assert len(pairs) >= 4 and st["batches"] == len(pairs), (st, sorted(pairs))
    assert st["flushed_drain"] == len(pairs) and st["rows_staged"] == 0
    # within a job completions come in submission order
    for p in pairs:
        mine = [x for (_, _, k, r, _), x in zip(tickets, order) if (_kclass(k), r) == p]
        assert mine == sorted(mine) and min(mine) >= 0
    bt.close()
    bt = open_batch(False, nwin + 1, max_delay_us=10 ** 9, max_symbol=64, arena=True)
    tickets = _run(bt, streams, poll=False)
    st0, plain, _ = _check(bt, o, streams, tickets)
    assert st0["batches"] > st["batches"] and st0["batches"] >= len({(k, r) for _, _, k, r, _ in tickets})
    assert all(np.array_equal(a, b) for x, y in zip(mixed, plain) for a, b in zip(x, y)) and len(mixed) == len(plain)
    assert st0["window_rows"] > st["window_rows"], "a change of length no longer ends a connection's run"
    bt.close()


def test_mixed_window_jobs_with_part_of_the_symbols_outside_the_arena(streams):
    """An arena of 1500 slots: the first 750 stream symbols (a struct and a data slot each) lie in it, the
    others and every repair come from the heap and go through the job's staging rows by device address."""
    bt = open_batch(True, 64, max_symbol=1500, arena=True, arena_bytes=1500 * 2112)
    o = Oracle()
    tickets = _run(bt, streams)
    st, _, _ = _check(bt, o, streams, tickets)
    assert st["rows_staged"] > 0 and st["rows_in_place"] > 0, st
    assert st["rows_staged"] + st["rows_in_place"] == st["window_rows"] + sum(r for _, _, _, r, _ in tickets), st
    bt.close()


def test_mixed_window_jobs_without_an_arena_are_all_staged(streams):
    """No registered heap: a mixed job still runs on row tables, every row through its staging rows."""
    bt = open_batch(True, 64, max_symbol=1500)
    o = Oracle()
    tickets = _run(bt, streams)
    st, _, _ = _check(bt, o, streams, tickets)
    assert st["rows_in_place"] == 0, st
    assert st["rows_staged"] == st["window_rows"] + sum(r for _, _, _, r, _ in tickets), st
    bt.close()


def test_the_switch_on_a_batcher_of_its_own():
    """pquic_fec_batch_set_window_mixed on an idle batcher: accepted both ways with this engine (it has the host
    form), refused without a batcher; declared in the header with the environment variable."""
    import ctypes as C
    root = os.path.join(os.path.dirname(__file__), "..")
    fec = C.CDLL(os.path.join(root, "pquic_amd", "lib", "libpquic_fec.so"))
    assert hasattr(fec, "fecgpu_rlc_window_encode_rows_var_host")
    assert fec.pquic_fec_batch_set_window_mixed(None, 1) == -1

    class Cfg(C.Structure):
        _fields_ = [("device", C.c_int), ("batch_blocks", C.c_uint32), ("max_delay_us", C.c_uint32),
                    ("max_symbol", C.c_uint32), ("nstreams", C.c_int), ("poll_blocks", C.c_uint32)]
    fec.pquic_fec_batcher_create.restype = C.c_void_p
    fec.pquic_fec_batcher_create.argtypes = [C.POINTER(Cfg)]
    fec.pquic_fec_batch_set_window_mixed.argtypes = [C.c_void_p, C.c_int]
    fec.pquic_fec_batcher_destroy.argtypes = [C.c_void_p]
    b = fec.pquic_fec_batcher_create(C.byref(Cfg(0, 8, 1000, 1200, 2, 0)))
    assert b
    try:
        assert fec.pquic_fec_batch_set_window_mixed(b, 1) == 0
        assert fec.pquic_fec_batch_set_window_mixed(b, 0) == 0
    finally:
        fec.pquic_fec_batcher_destroy(b)
    text = open(os.path.join(root, "include", "pquic_fec_batch.h")).read()
    assert "pquic_fec_batch_set_window_mixed(" in text and ENV in text
