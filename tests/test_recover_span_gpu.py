"""The blocking span recovery call (pquic_fec_rlc_recover_span) on the device, through the span receiver
stand-in tools/libspanload.so at MAXL 64.  Spans are coded by the numpy model (span_model.py), which is also
the ground truth for what is determined; the original sources are the ground truth for the bytes.  Every span
goes through the blocking call and through the batcher (pquic_fec_batch_recover_span): the same symbols."""
import ctypes as C

import numpy as np
import pytest

from span_model import RECOVERED, SINGULAR
from test_batch_span_gpu import MAXL, Driver, Span, libs, model  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_UNBOUND = 0x41B
FIVE = [(5 * o, 30, 1) for o in range(5)]
BASE = 0x100000000 - 20  # the ids wrap inside every span


def cases(model):
    """(a), (b), (c), (g), (i) of the one-launch kernel's cases, ragged, as the receiver would hold them"""
    rng = np.random.default_rng(4)

    def lens(K):
        n = rng.integers(1, MAXL + 1, K)
        n[rng.integers(0, K)] = MAXL
        return n

    out = {
        "a": Span(model, 50, FIVE, 1, lens=lens(50)).lose([22, 23]),
        "b": Span(model, 50, FIVE, 2, lens=lens(50)).lose([22, 23, 48, 49]),
        "c": Span(model, 50, FIVE, 3, lens=lens(50)).lose([0, 1]),
        "g": Span(model, 64, [(0, 64, 12)], 4, lens=lens(64), zero_cols=[9]).lose(range(3, 31, 3)),
        "i": Span(model, 125, [(5 * o, 30, 1) for o in range(20)], 5, lens=lens(125)).lose([40, 41, 42, 90, 91]),
    }
    for sp in out.values():
        sp.solve(model)
    a, b, c, g, i = (out[x] for x in "abcgi")
    assert np.nonzero(a.det)[0].tolist() == [22, 23] and not a.alone.any()
    assert np.nonzero(b.det)[0].tolist() == [22, 23] and b.status == RECOVERED
    assert c.status == SINGULAR and not c.exp
    assert g.det.sum() == 10 and g.det[9] and 9 not in g.exp and len(g.exp) == 9  # the zero source is not handed over
    assert i.det.sum() == 5 and not i.alone.any()
    return out


class Blocking(Driver):
    def __init__(self, libs, registered):
        super().__init__(libs, 1, [registered])
        d = self.d
        d.sl_recover_span.restype = C.c_long
        d.sl_recover_span.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int]
        self.eng.pquic_fec_hook_rows_stats.argtypes = [C.c_void_p]

    def rows(self):
        out = (C.c_uint64 * 4)()
        self.eng.pquic_fec_hook_rows_stats(out)
        return list(out)

    def recover(self, sp, fault=0, K=None, R=None, first=None, nss=None, rep_ids=None):
        first = sp.first if first is None else np.asarray(first, np.uint32)
        nss = sp.wlen if nss is None else np.asarray(nss, np.uint8)
        rep_ids = sp.rep_ids if rep_ids is None else np.asarray(rep_ids, np.int64)
        src_ids = np.concatenate([sp.src_ids, np.full(200, -1, np.int64)])
        rep_ids = np.concatenate([rep_ids, np.full(200, -1, np.int64)])
        first = np.concatenate([first, np.zeros(200, np.uint32)])
        nss = np.concatenate([nss, np.ones(200, np.uint8)])
        return self.d.sl_recover_span(self.h, sp.conn, sp.base & 0xFFFFFFFF, sp.K if K is None else K,
                                      sp.got.size if R is None else R, src_ids.ctypes.data, rep_ids.ctypes.data,
                                      first.ctypes.data, nss.ctypes.data, fault)

    def cols(self, t):
        ncols = self.ticket(t)[4]
        col, fpid, ln = (np.zeros(max(ncols, 1), np.uint32) for _ in range(3))
        data = np.zeros((max(ncols, 1), MAXL), np.uint8)
        self.d.sl_ticket_cols(self.h, t, col.ctypes.data, fpid.ctypes.data, ln.ctypes.data, data.ctypes.data, MAXL)
        return col[:ncols].tolist(), fpid[:ncols].tolist(), ln[:ncols].tolist(), data[:ncols].tobytes()


@pytest.mark.parametrize("registered", [1, 0])
@pytest.mark.parametrize("name", ["a", "b", "c", "g", "i"])
def test_blocking_call_equals_the_model_and_the_batcher(libs, model, name, registered):
    sp = cases(model)[name]
    eng = libs[0]
    with Blocking(libs, registered) as drv:
        drv.build(sp, 0, BASE)
        baseline = drv.live()
        rows0, sing0 = drv.rows(), eng.pquic_fec_singular_blocks()
        t = drv.recover(sp)
        assert t >= 0
        rows1 = drv.rows()
        # column, fpid.raw = base_id + column mod 2^32, data_length = the longest received repair, bytes
        drv.check(t, sp)
        assert (BASE + sp.K) > 0xFFFFFFFF and sp.maxl == int(sp.rep_len[sp.got].max())
        nrows = sp.K + sp.got.size  # every source (received or allocated for a missing column) and every repair
        moved = [rows1[x] - rows0[x] for x in range(4)]
        assert moved == ([nrows, 0, 0, 1] if registered else [0, nrows, 0, 1])
        assert eng.pquic_fec_singular_blocks() - sing0 == (1 if name == "c" else 0)
        if name == "c":
            assert drv.ticket(t)[2:] == [0, 0, 0]  # ret 0, nrecovered 0, no column
        # the same span through the batcher: the same symbols
        t2 = drv.submit(sp)
        assert t2 >= 0
        drv.d.sl_drain(drv.h)
        drv.check(t2, sp)
        assert drv.cols(t2) == drv.cols(t)
        for x in (t, t2):
            drv.d.sl_release(drv.h, x)
        assert drv.live() == baseline  # what was not recovered was freed by the call, the rest by its owner


def test_refusals_allocate_nothing(libs, model):
    sp = cases(model)["a"]
    with Blocking(libs, 1) as drv:
        drv.build(sp, 0, BASE)
        baseline = drv.live()
        R = sp.got.size
        bad_first = sp.first.copy()
        bad_first[2] = (BASE + 21) & 0xFFFFFFFF  # 21 + 30 > 50: leaves the span
        before = (BASE - 1) & 0xFFFFFFFF         # offset 2^32 - 1
        no_rep = sp.rep_ids.copy()
        no_rep[1] = -1
        zero_nss = sp.wlen.copy()
        zero_nss[4] = 0
        for kw in ([dict(fault=f) for f in (1, 2, 3, 4, 6, 7, 8)] +
                   [dict(K=0), dict(K=129), dict(R=0), dict(R=129), dict(first=bad_first), dict(nss=zero_nss),
                    dict(first=[before] + sp.first[1:].tolist()), dict(rep_ids=no_rep), dict(K=29)]):
            assert drv.recover(sp, **kw) == -1, kw
            assert drv.live() == baseline, kw
        assert R == 5
        # a span with no missing column: 0, nothing recovered, nothing allocated
        whole = Span(model, 50, FIVE, 9).solve(model)
        drv.build(whole, 0, 1000)
        baseline = drv.live()
        rows0 = drv.rows()
        t = drv.recover(whole)
        assert t >= 0 and drv.ticket(t)[2:] == [0, 0, 0] and drv.live() == baseline and drv.rows() == rows0


def test_window_by_window_recovers_nothing(libs, model):
    """Case (a) through pquic_fec_rlc_recover, one window at a time in full-rank mode: every window holds both
    losses under its one repair, so nothing is recovered -- what the span call is for."""
    from test_protoops_gpu import Host
    sp = cases(model)["a"]
    assert libs[0].pquic_fec_get_recover_mode() == 0
    host = Host()  # binds the mini host's allocator (a stand-in that closed has unbound its own)
    libs[0].pquic_fec_set_recover_mode.argtypes = [C.c_int]
    assert libs[0].pquic_fec_set_recover_mode(1) == 0
    try:
        for w, (o, n, _) in enumerate(FIVE):
            srcs = [sp.src[o + j, :sp.len[o + j]].copy() if sp.present[o + j] else None for j in range(n)]
            reps = [sp.rep[w, :sp.rep_len[w]].copy()]
            ret, rec, cur = host.recover(False, (BASE + o) & 0xFFFFFF, srcs, reps, [0])
            assert ret == 0 and rec == {} and cur == n - 2, w
    finally:
        assert libs[0].pquic_fec_set_recover_mode(0) == 0
