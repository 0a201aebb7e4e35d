"""Span jobs of the batching adapter (pquic_fec_batch_recover_span) on the device, through the span receiver
stand-in tools/libspanload.so.  Spans are coded by the numpy model (span_model.py), which is also the ground
truth for what is determined; the original sources are the ground truth for the bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from span_model import SpanModel, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAXL = 64


@pytest.fixture(scope="module")
def libs():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    eng = C.CDLL(os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so"))
    eng.fecgpu_set_knob.argtypes = [C.c_char_p, C.c_int]
    eng.pquic_fec_singular_blocks.restype = C.c_uint64
    d = C.CDLL(os.path.join(ROOT, "tools", "libspanload.so"))
    d.sl_open.restype = C.c_void_p
    d.sl_open.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_size_t, C.c_char_p]
    d.sl_close.argtypes = [C.c_void_p]
    d.sl_live.restype = C.c_long
    d.sl_live.argtypes = [C.c_void_p, C.c_int]
    for f in (d.sl_source, d.sl_repair, d.sl_submit):
        f.restype = C.c_long
    d.sl_source.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint, C.c_uint32]
    d.sl_repair.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint, C.c_uint32, C.c_uint32]
    d.sl_submit.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    d.sl_poll.argtypes = [C.c_void_p, C.c_uint64]
    d.sl_drain.argtypes = [C.c_void_p]
    d.sl_ticket.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    d.sl_ticket_cols.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    d.sl_release.argtypes = [C.c_void_p, C.c_long]
    d.sl_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return eng, d


@pytest.fixture(scope="module")
def model():
    return SpanModel()


STATS = ("submitted completed batches flushed_full flushed_deadline flushed_drain immediate engine_errors windows "
         "window_rows engine_us stage_us complete_us rows_in_place rows_staged jobs_allocated job_alloc_us "
         "deadline_holds spans span_symbols").split()


class Span:
    """One span: K columns of ragged sources under windows [(off, nss, r)], coded by the model; `present` /
    `rpresent` say what the receiver holds.  exp: column -> bytes of every symbol a completion must hand over."""

    def __init__(self, model, K, windows, seed, lens=None, zero_cols=()):
        rng = np.random.default_rng(seed)
        self.K, self.windows = K, windows
        self.len = np.full(K, MAXL) if lens is None else np.asarray(lens)
        self.src = rng.integers(1, 256, (K, MAXL), dtype=np.uint8)
        self.src[list(zero_cols)] = 0
        self.src[np.arange(MAXL)[None, :] >= self.len[:, None]] = 0
        self.seed = np.concatenate([np.arange(r) for _, _, r in windows]).astype(np.uint32)[None]
        self.off = np.concatenate([np.full(r, o) for o, _, r in windows]).astype(np.uint8)[None]
        self.nss = np.concatenate([np.full(r, n) for _, n, r in windows]).astype(np.uint8)[None]
        self.R = self.seed.shape[1]
        every = model.solve(K, self.seed, self.off, self.nss, pack(np.ones((1, K), bool)), pack(np.ones((1, self.R), bool)))
        self.rep = model.encode(every, self.src[None])[0]
        # each repair as long as the longest source of its window
        self.rep_len = np.array([self.len[o:o + n].max() for o, n in zip(self.off[0], self.nss[0])])
        self.present = np.ones(K, bool)
        self.rpresent = np.ones(self.R, bool)

    def lose(self, cols=(), reps=()):
        self.present[list(cols)] = False
        self.rpresent[list(reps)] = False
        return self

    def solve(self, model):
        got = np.nonzero(self.rpresent)[0]
        self.got = got
        self.maxl = int(self.rep_len[got].max()) if got.size else 0
        s = model.solve(self.K, self.seed[:, got], self.off[:, got], self.nss[:, got], pack(self.present[None]),
                        pack(np.ones((1, got.size), bool)))
        self.det = s.det[0]
        self.status = int(s.status[0])
        self.alone = model.windows_alone(s, self.off[:, got], self.nss[:, got], propagate=True)[0]
        self.exp = {int(c): self.src[c, :self.maxl] for c in np.nonzero(self.det)[0] if self.src[c, :self.maxl].any()}
        return self


class Driver:
    def __init__(self, libs, nconn=1, registered=None, batch_blocks=128, max_delay_us=1000000, arena=8 << 20):
        self.eng, self.d = libs
        reg = bytes(registered if registered is not None else [1] * nconn)
        self.h = self.d.sl_open(0, batch_blocks, max_delay_us, MAXL, 0, nconn, arena, reg)
        assert self.h
        self.tickets = []

    def close(self):
        if self.h:
            self.d.sl_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        w = (C.c_uint64 * len(STATS))()
        assert self.d.sl_stats(self.h, w, len(STATS)) == 8 * len(STATS)
        return dict(zip(STATS, w))

    def live(self):
        return self.d.sl_live(self.h, -1)

    def build(self, sp, conn, base_id):
        """the receiver's symbols of span sp"""
        sp.conn, sp.base = conn, base_id
        sp.src_ids = np.full(sp.K, -1, np.int64)
        for c in np.nonzero(sp.present)[0]:
            n = int(min(sp.len[c], MAXL))
            sp.src_ids[c] = self.d.sl_source(self.h, conn, sp.src[c, :n].tobytes(), n, (base_id + int(c)) & 0xFFFFFFFF)
        sp.rep_ids = np.array([self.d.sl_repair(self.h, conn, sp.rep[i, :sp.rep_len[i]].tobytes(), int(sp.rep_len[i]),
                                                int(sp.seed[0, i]), (base_id + int(sp.off[0, i])) & 0xFFFFFFFF)
                               for i in sp.got], np.int64)
        assert (sp.src_ids[sp.present] >= 0).all() and (sp.rep_ids >= 0).all()
        sp.first = ((base_id + sp.off[0, sp.got].astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
        sp.wlen = np.ascontiguousarray(sp.nss[0, sp.got])

    def submit(self, sp, now=1000, fault=0, K=None, R=None, first=None, nss=None, rep_ids=None):
        first = sp.first if first is None else np.asarray(first, np.uint32)
        nss = sp.wlen if nss is None else np.asarray(nss, np.uint8)
        rep_ids = sp.rep_ids if rep_ids is None else np.asarray(rep_ids, np.int64)
        src_ids = np.concatenate([sp.src_ids, np.full(200, -1, np.int64)])
        rep_ids = np.concatenate([rep_ids, np.full(200, -1, np.int64)])
        first = np.concatenate([first, np.zeros(200, np.uint32)])
        nss = np.concatenate([nss, np.ones(200, np.uint8)])
        t = self.d.sl_submit(self.h, sp.conn, sp.base & 0xFFFFFFFF, sp.K if K is None else K,
                             sp.got.size if R is None else R, src_ids.ctypes.data, rep_ids.ctypes.data,
                             first.ctypes.data, nss.ctypes.data, now, fault)
        if t >= 0:
            self.tickets.append((t, sp))
        return t

    def ticket(self, t):
        out = (C.c_int64 * 5)()
        self.d.sl_ticket(self.h, t, out)
        return list(out)

    def check(self, t, sp):
        """the completion of ticket t against the model and the original bytes"""
        done, order, ret, nrec, ncols = self.ticket(t)
        assert done == 1 and ret == 0
        assert nrec == ncols == len(sp.exp), (t, nrec, ncols, sorted(sp.exp))
        col, fpid, ln = (np.zeros(max(ncols, 1), np.uint32) for _ in range(3))
        data = np.zeros((max(ncols, 1), MAXL), np.uint8)
        self.d.sl_ticket_cols(self.h, t, col.ctypes.data, fpid.ctypes.data, ln.ctypes.data, data.ctypes.data, MAXL)
        assert col[:ncols].tolist() == sorted(sp.exp)
        for x in range(ncols):
            c = int(col[x])
            assert ln[x] == sp.maxl and fpid[x] == (sp.base + c) & 0xFFFFFFFF
            assert np.array_equal(data[x, :sp.maxl], sp.exp[c]), (t, c)
        return order

    def finish(self, baseline):
        """drain, check every ticket, hand the symbols back: the allocator is where it was"""
        self.d.sl_drain(self.h)
        orders = [self.check(t, sp) for t, sp in self.tickets]
        for t, _ in self.tickets:
            self.d.sl_release(self.h, t)
        assert self.live() == baseline
        return orders


NEIGHBOUR = [(2 * w, 6, 1) for w in range(6)]  # k6 r1 step 2: spans of 16 columns


def neighbour_spans(model, n=40):
    """two losses in columns that always share their windows: no window alone recovers either"""
    pairs = [(6, 7), (8, 9), (4, 5), (6, 7), (8, 9)]
    out = []
    for i in range(n):
        sp = Span(model, 16, NEIGHBOUR, 500 + i).lose(pairs[i % len(pairs)]).solve(model)
        assert sp.det.sum() == 2 and not sp.alone.any()
        out.append(sp)
    return out


def run_neighbours(libs, model, registered):
    bases = [7, 0x100000000 - 5, 123456]
    with Driver(libs, 3, registered) as drv:
        spans = neighbour_spans(model)
        for i, sp in enumerate(spans):
            drv.build(sp, i % 3, bases[i % 3] + 16 * (i // 3))
        baseline = drv.live()
        for sp in spans:
            assert drv.submit(sp) >= 0
        orders = drv.finish(baseline)
        assert orders == list(range(len(spans)))  # one completion per span, in submission order
        st = drv.stats()
    assert st["engine_errors"] == 0 and st["spans"] == 40 and st["span_symbols"] == 80 and st["batches"] == 1
    assert st["submitted"] == st["completed"] == 40
    return st


def test_neighbour_recovery_in_place(libs, model):
    st = run_neighbours(libs, model, [1, 1, 1])
    assert st["rows_staged"] == 0 and st["rows_in_place"] == 40 * (16 + 6)


def test_staged_and_mixed(libs, model):
    st = run_neighbours(libs, model, [0, 0, 0])
    assert st["rows_in_place"] == 0 and st["rows_staged"] == 40 * (16 + 6)
    st = run_neighbours(libs, model, [1, 0, 1])
    assert st["rows_in_place"] > 0 and st["rows_staged"] > 0


def test_knob_parity(libs, model):
    eng = libs[0]
    assert eng.fecgpu_set_knob(b"span_compact", 0) == 0
    try:
        run_neighbours(libs, model, [1, 0, 1])
    finally:
        assert eng.fecgpu_set_knob(b"span_compact", 1) == 0


def test_ragged_lengths_and_a_zero_source(libs, model):
    rng = np.random.default_rng(77)
    with Driver(libs, 2) as drv:
        spans = []
        for i in range(24):
            lens = rng.integers(1, MAXL + 1, 16)
            lens[i % 16] = 1 + (i * 7) % MAXL
            sp = Span(model, 16, NEIGHBOUR, 900 + i, lens=lens, zero_cols=[6] if i % 4 == 0 else ())
            spans.append(sp.lose([(6, 7), (8, 9), (3, 12)][i % 3], [5] if i % 5 == 0 else ()).solve(model))
        zero = [sp for sp in spans if sp.det[6] and not sp.src[6].any() and not sp.present[6]]
        assert zero and all(6 not in sp.exp for sp in zero)  # determined, all zero: not handed over
        assert len({sp.maxl for sp in spans}) >= 3 and all(sp.len[sp.present].min() < sp.maxl for sp in spans)
        for i, sp in enumerate(spans):
            drv.build(sp, i % 2, 1000 * i)
        baseline = drv.live()
        for sp in spans:
            assert drv.submit(sp) >= 0
        drv.finish(baseline)  # the zero source's pre-allocation went back: live allocations at the baseline
        st = drv.stats()
    assert st["rows_staged"] == 0 and st["engine_errors"] == 0


def test_mixed_shapes_share_one_batcher(libs, model):
    eng = libs[0]
    spans = [
        Span(model, 5, [(0, 5, 1)], 1).lose([1, 3]),                                    # singular: queue (64, 8)
        Span(model, 5, [(0, 5, 1)], 2),                                                 # nothing missing
        Span(model, 64, [(0, 8, 2), (8, 56, 1)], 3).lose([1, 6, 10, 20, 30]),          # more losses than repairs: (64, 8)
        Span(model, 64, [(8 * w, 8, 1) for w in range(8)], 4).lose([0, 9, 63]),         # K 64 R 8
        Span(model, 65, [(7 * w, 9, 1) for w in range(9)], 5).lose([2, 30, 64]),        # K 65 R 9: (128, 32)
        Span(model, 128, [(3 * w, 32, 1) for w in range(33)], 6).lose([5, 6, 70, 127]),  # K 128 R 33: (128, 128)
        Span(model, 128, [(0, 128, 128)], 7).lose(range(3, 120, 6)),                    # K 128 R 128
        Span(model, 64, [(0, 64, 9)], 8).lose(range(0, 64, 8)),                         # K 64 R 9: (64, 32)
        Span(model, 5, [(0, 5, 1)], 9).lose([4]),                                       # K 5 R 1, recovered
    ]
    for sp in spans:
        sp.solve(model)
    assert spans[0].status == 3 and not spans[0].exp
    assert sorted(spans[2].exp) == [1, 6] and (~spans[2].present).sum() > spans[2].R
    assert len(spans[6].exp) == 20 and len(spans[7].exp) == 8 and sorted(spans[8].exp) == [4]
    queues = {(64 if sp.K <= 64 else 128, 8 if sp.got.size <= 8 else 32 if sp.got.size <= 32 else 128)
              for sp in spans if not sp.present.all()}
    assert len(queues) == 4
    with Driver(libs, 2, arena=16 << 20) as drv:
        for i, sp in enumerate(spans):
            drv.build(sp, i % 2, 4096 * i)
        baseline = drv.live()
        sing0 = eng.pquic_fec_singular_blocks()
        for i, sp in enumerate(spans):
            t = drv.submit(sp)
            assert t >= 0
            if i == 1:  # nothing missing: completed inside the call
                assert drv.ticket(t)[:4] == [1, 0, 0, 0] and drv.stats()["immediate"] == 1
        drv.finish(baseline)
        st = drv.stats()
        assert eng.pquic_fec_singular_blocks() == sing0 + 1
    assert st["batches"] == len(queues) and st["spans"] == len(spans) - 1 and st["engine_errors"] == 0
    assert st["rows_staged"] == 0


def test_argument_errors(libs, model):
    with Driver(libs, 1) as drv:
        sp = Span(model, 16, NEIGHBOUR, 11).lose([6, 7]).solve(model)
        drv.build(sp, 0, 100)
        long_sp = Span(model, 16, NEIGHBOUR, 12).lose([6, 7]).solve(model)
        drv.build(long_sp, 0, 200)
        long_id = drv.d.sl_source(drv.h, 0, bytes(MAXL + 1), MAXL + 1, 200)  # longer than max_symbol
        baseline = drv.live()
        bad = [dict(K=0), dict(K=129), dict(R=0), dict(R=129),
               dict(nss=[0] + [6] * 5),                                   # an empty window
               dict(first=np.concatenate([sp.first[:5], [100 + 11]])),    # 11 + 6 > 16: past the span
               dict(first=np.concatenate([[99], sp.first[1:]])),          # starts below the span
               dict(rep_ids=[-1] + sp.rep_ids[1:].tolist())]              # a NULL repair
        bad += [dict(fault=f) for f in range(1, 7)]
        for kw in bad:
            assert drv.submit(sp, **kw) == -1, kw
        long_sp.src_ids[0] = long_id
        assert drv.submit(long_sp) == -1
        st = drv.stats()
        assert st["submitted"] == 0 and st["immediate"] == 0 and drv.live() == baseline
        assert drv.d.sl_drain(drv.h) == 0


def test_deadline_flush_and_job_reuse(libs, model):
    spans = neighbour_spans(model, 129)
    with Driver(libs, 1, batch_blocks=128, max_delay_us=1000, arena=16 << 20) as drv:
        for i, sp in enumerate(spans):
            drv.build(sp, 0, 16 * i)
        baseline = drv.live()
        assert drv.submit(spans[0], now=5000) >= 0
        assert drv.d.sl_poll(drv.h, 5999) == 0 and drv.stats()["flushed_deadline"] == 0
        drv.d.sl_poll(drv.h, 6001)  # past max_delay_us: flushed by the deadline
        assert drv.stats()["flushed_deadline"] == 1
        drv.d.sl_drain(drv.h)
        assert drv.ticket(0)[0] == 1
        for sp in spans[1:]:  # the same queue again, now a full job
            assert drv.submit(sp, now=7000) >= 0
        st = drv.stats()
        assert st["flushed_full"] == 1 and st["batches"] == 2
        orders = drv.finish(baseline)
        assert orders == list(range(129))
        assert drv.stats()["spans"] == 129
