"""Span decode without a GPU: fecgpu_rlc_span_layout (pure host code), the exported entry points, argument
errors refused before any device call, and the numpy model (span_model.py) against the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle_py import Oracle, synth_bytes
from span_model import NOTHING, RECOVERED, SINGULAR, SpanModel, pack

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")

v, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
OK, ERR_INVALID = 0, -1
NAMES = ("fecgpu_rlc_span_decode_plan", "fecgpu_rlc_span_decode", "fecgpu_rlc_span_decode_rows_fused",
         "fecgpu_rlc_span_decode_rows_fused_host", "fecgpu_rlc_span_layout")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = C.CDLL(LIB)
    L.fecgpu_rlc_decode_workspace.restype = sz
    L.fecgpu_rlc_decode_workspace.argtypes = [u64, u32, u32]
    L.fecgpu_last_error.restype = C.c_char_p
    return L


def layout(first_id, nss):
    from pquic_amd import span_layout
    return span_layout(np.array(first_id, np.uint32), np.array(nss, np.uint8))


# ---------------------------------------------------------------- span_layout
def test_span_layout_plain():
    base, K, off = layout([100, 105, 110], [30, 30, 30])
    assert (base, K, off.tolist()) == (100, 40, [0, 5, 10])
    base, K, off = layout([7], [1])
    assert (base, K, off.tolist()) == (7, 1, [0])
    base, K, off = layout([10, 10, 12], [4, 8, 2])  # windows of several lengths, one start twice
    assert (base, K, off.tolist()) == (10, 8, [0, 0, 2])


def test_span_layout_unordered_starts():
    base, K, off = layout([110, 100, 105, 100], [30, 30, 30, 5])
    assert (base, K, off.tolist()) == (100, 40, [10, 0, 5, 0])


def test_span_layout_ids_across_the_wrap():
    top = 1 << 32
    base, K, off = layout([top - 10, top - 5, 0, 5], [30, 30, 30, 30])
    assert (base, K, off.tolist()) == (top - 10, 45, [0, 5, 10, 15])
    base, K, off = layout([3, top - 7, top - 2], [20, 20, 20])  # the first repair lies past the wrap
    assert (base, K, off.tolist()) == (top - 7, 30, [10, 0, 5])


def test_span_layout_width_limit_and_empty(lib):
    from pquic_amd import FecGpuError
    base, K, off = layout([0, 98], [30, 30])
    assert (K, off.tolist()) == (128, [0, 98])
    with pytest.raises(FecGpuError, match="128"):
        layout([0, 99], [30, 30])
    with pytest.raises(FecGpuError, match="128"):
        layout([5, 1 << 31], [30, 30])
    with pytest.raises(FecGpuError, match="no repair"):
        layout([], [])
    f = lib.fecgpu_rlc_span_layout
    f.argtypes = [v, v, u32, v, v, v]
    ids, n, out = np.zeros(2, np.uint32), np.ones(2, np.uint8), np.zeros(4, np.uint32)
    assert f(ids.ctypes.data, n.ctypes.data, 0, out.ctypes.data, out.ctypes.data + 4, out.ctypes.data + 8) == ERR_INVALID
    assert f(None, n.ctypes.data, 2, out.ctypes.data, out.ctypes.data + 4, out.ctypes.data + 8) == ERR_INVALID
    assert f(ids.ctypes.data, n.ctypes.data, 2, out.ctypes.data, None, out.ctypes.data + 8) == ERR_INVALID


# ---------------------------------------------------------------- the library
def test_symbols_exported_and_declared(lib):
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
    import pquic_amd
    for name in ("rlc_span_decode_plan", "rlc_span_decode", "rlc_span_decode_rows_fused"):
        assert hasattr(pquic_amd.Engine, name)
    assert hasattr(pquic_amd.HostPath, "rlc_span_decode_rows_fused")
    assert "span_layout" in pquic_amd.__all__


def refused(lib, rc, word):
    assert rc == ERR_INVALID
    assert word in lib.fecgpu_last_error().decode(), lib.fecgpu_last_error()


def test_plan_argument_errors_without_device(lib):
    f = lib.fecgpu_rlc_span_decode_plan
    f.argtypes = [u64, u32, u32, v, v, v, v, v, v, sz, v]
    big = 1 << 30
    # nspans, K, R, rep_seed, rep_off, rep_nss, sp, rp, ws, wsb, stream
    assert f(0, 55, 6, None, None, None, None, None, None, 0, None) == OK  # empty
    refused(lib, f(1, 0, 6, 16, 16, 16, 16, 16, 16, big, None), "K out of range")
    refused(lib, f(1, 129, 6, 16, 16, 16, 16, 16, 16, big, None), "K out of range")
    refused(lib, f(1, 55, 0, 16, 16, 16, 16, 16, 16, big, None), "R out of range")
    refused(lib, f(1, 55, 129, 16, 16, 16, 16, 16, 16, big, None), "R out of range")
    refused(lib, f(1, 55, 6, None, 16, 16, 16, 16, 16, big, None), "NULL")
    refused(lib, f(1, 55, 6, 16, None, 16, 16, 16, 16, big, None), "NULL")
    refused(lib, f(1, 55, 6, 16, 16, None, 16, 16, 16, big, None), "NULL")
    refused(lib, f(1, 55, 6, 16, 16, 16, None, 16, 16, big, None), "NULL")
    refused(lib, f(1, 55, 6, 16, 16, 16, 16, None, 16, big, None), "NULL")
    refused(lib, f(1, 55, 6, 16, 16, 16, 16, 16, None, big, None), "NULL")
    refused(lib, f(1, 55, 6, 18, 16, 16, 16, 16, 16, big, None), "aligned")
    refused(lib, f(1, 55, 6, 16, 17, 19, 20, 16, 16, big, None), "aligned")  # u8 tables need none, masks 8
    refused(lib, f(1, 55, 6, 16, 17, 19, 16, 16, 24, big, None), "aligned")
    need = lib.fecgpu_rlc_decode_workspace(8, 55, 6)
    refused(lib, f(8, 55, 6, 16, 16, 16, 16, 16, 16, need - 1, None), "workspace")


def test_decode_argument_errors_without_device(lib):
    f = lib.fecgpu_rlc_span_decode
    f.argtypes = [v, v, u64, u32, u32, u32, v, v, v, v, v, v, v, v, sz, v]
    big = 1 << 30
    # src, rep, nspans, K, R, L, rep_seed, rep_off, rep_nss, sp, rp, status, recovered, ws, wsb, stream
    assert f(None, None, 0, 55, 6, 1200, None, None, None, None, None, None, None, None, 0, None) == OK
    refused(lib, f(None, 16, 1, 55, 6, 1200, 16, 16, 16, 16, 16, 16, 16, 16, big, None), "NULL")
    refused(lib, f(16, None, 1, 55, 6, 1200, 16, 16, 16, 16, 16, 16, 16, 16, big, None), "NULL")
    refused(lib, f(16, 16, 1, 55, 6, 1200, 16, 16, 16, 16, 16, None, 16, 16, big, None), "NULL")
    refused(lib, f(16, 16, 1, 55, 6, 1200, 16, 16, 16, 16, 16, 16, None, 16, big, None), "NULL")
    refused(lib, f(16, 16, 1, 55, 6, 1200, 16, 16, None, 16, 16, 16, 16, 16, big, None), "NULL")
    refused(lib, f(16, 16, 1, 55, 6, 1201, 16, 16, 16, 16, 16, 16, 16, 16, big, None), "multiple of 4")
    refused(lib, f(18, 16, 1, 55, 6, 1200, 16, 16, 16, 16, 16, 16, 16, 16, big, None), "aligned")
    refused(lib, f(16, 16, 1, 129, 6, 1200, 16, 16, 16, 16, 16, 16, 16, 16, big, None), "K out of range")
    refused(lib, f(16, 16, 1, 55, 130, 1200, 16, 16, 16, 16, 16, 16, 16, 16, big, None), "R out of range")
    need = lib.fecgpu_rlc_decode_workspace(3, 55, 6)
    refused(lib, f(16, 16, 3, 55, 6, 1200, 16, 16, 16, 16, 16, 16, 16, 16, need - 1, None), "workspace")


def test_rows_fused_argument_errors_without_device(lib):
    f = lib.fecgpu_rlc_span_decode_rows_fused
    f.argtypes = [v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v, v, v, v, sz, v]
    big = 1 << 30
    # src_rows, src_len, rep_rows, rep_len, blk_len, nspans, K, R, L, seed, off, nss, sp, rp, st, rec, ws, wsb, stream
    ok = [16, 16, 16, 16, 16, 1, 55, 6, 1200, 16, 16, 16, 16, 16, 16, 16, 16, big, None]
    assert f(*[None] * 5, 0, 55, 6, 1200, *[None] * 8, 0, None) == OK
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16):
        a = list(ok)
        a[i] = None
        refused(lib, f(*a), "NULL")
    for i, bad in ((0, 20), (1, 18), (9, 18), (12, 20), (15, 20), (16, 24)):
        a = list(ok)
        a[i] = bad
        refused(lib, f(*a), "aligned")
    for i, bad, word in ((6, 0, "K out of range"), (6, 129, "K out of range"), (7, 0, "R out of range"),
                         (7, 129, "R out of range"), (8, 1202, "multiple of 4"), (17, 15, "workspace")):
        a = list(ok)
        a[i] = bad
        refused(lib, f(*a), word)


def test_host_form_checks_before_any_launch(lib):
    f = lib.fecgpu_rlc_span_decode_rows_fused_host
    f.argtypes = [v, v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v, v, v]
    K, R, L = 8, 2, 64
    rows = np.full(K, 4096, np.uint64)
    slen = np.full(K, 64, np.uint32)
    rrows = np.full(R, 4096, np.uint64)
    rlen = np.full(R, 64, np.uint32)
    blen = np.array([64], np.uint32)
    seed = np.zeros(R, np.uint32)
    off = np.array([0, 4], np.uint8)
    nss = np.array([8, 4], np.uint8)
    sp = np.array([0xFE, 0], np.uint64)
    rp = np.array([3, 0], np.uint64)
    st, rec = np.zeros(1, np.uint8), np.zeros(2, np.uint64)

    def call(ctx=None, **kw):
        a = dict(rows=rows, slen=slen, rrows=rrows, rlen=rlen, blen=blen, seed=seed, off=off, nss=nss, sp=sp, rp=rp)
        a.update(kw)
        p = {k_: (None if x is None else x.ctypes.data) for k_, x in a.items()}
        return f(ctx, p["rows"], p["slen"], p["rrows"], p["rlen"], p["blen"], 1, K, R, L, p["seed"], p["off"],
                 p["nss"], p["sp"], p["rp"], st.ctypes.data, rec.ctypes.data)

    refused(lib, call(), "context")  # everything else in order: only the context is missing
    refused(lib, call(off=None), "NULL")
    refused(lib, call(nss=None), "NULL")
    refused(lib, call(nss=np.array([8, 5], np.uint8)), "rep_off + rep_nss")
    refused(lib, call(nss=np.array([8, 5], np.uint8), rp=np.array([1, 0], np.uint64)), "context")  # absent: not checked
    refused(lib, call(blen=np.array([68], np.uint32)), "blk_len")
    refused(lib, call(slen=np.full(K, 65, np.uint32) * np.array([0] + [1] * 7, np.uint32)), "src_len")


# ---------------------------------------------------------------- the model against the oracle
def test_model_matches_oracle_on_full_width_repairs():
    """off = 0, nss = K: wherever the oracle's fec_recover replay recovers a block, the model determines
    every missing source and computes the oracle's bytes from the received symbols alone."""
    o = Oracle()
    m = SpanModel(o)
    K, R, L, nb = 12, 5, 32, 60
    rng = np.random.default_rng(20260)
    src = synth_bytes(nb * K * L, 77).reshape(nb, K, L).copy()
    seed = rng.integers(1, 1 << 24, (nb, R)).astype(np.uint32)
    off = np.zeros((nb, R), np.uint8)
    nss = np.full((nb, R), K, np.uint8)
    present = np.ones((nb, K), bool)
    for b in range(nb):
        present[b, rng.choice(K, int(rng.integers(1, 5)), replace=False)] = False
    rpres = rng.random((nb, R)) < 0.8
    s = m.solve(K, seed, off, nss, pack(present), pack(rpres), with_T=True)
    rep = m.encode(s, src)  # absent rows are zero rows of C: their repairs are never used
    work = np.where(present[:, :, None], src, 0xA5).astype(np.uint8)
    out = m.solve_bytes(s, work, rep)
    seen = 0
    for b in range(nb):
        st, got = o.rlc_decode_block(0, [src[b, j] if present[b, j] else None for j in range(K)],
                                     [rep[b, i] if rpres[b, i] else None for i in range(R)], rep_seeds=seed[b])
        if st != 0:
            continue
        seen += 1
        assert s.status[b] == RECOVERED and (s.det[b] == ~present[b]).all(), b
        for j, x in got.items():
            assert np.array_equal(out[b, j], x[:L]), (b, j)
        assert np.array_equal(out[b], src[b]), b
    assert seen >= 20


def test_model_partial_and_status_rules():
    """Two windows on a span: the cluster with enough repairs is determined, the other is not; no determined
    column: SINGULAR; n == 0 or m == 0: NOTHING; an invalid descriptor counts as absent."""
    m = SpanModel()
    K = 12
    seed = np.array([[1, 2, 3]] * 5, np.uint32)
    off = np.array([[0, 0, 6]] * 5, np.uint8)
    nss = np.array([[6, 6, 6]] * 5, np.uint8)
    nss[4, 2] = 7  # leaves the span
    pres = np.ones((5, K), bool)
    pres[0, [1, 2, 7, 8]] = False   # cluster one: two repairs; cluster two: one repair for two losses
    pres[1, [7, 8]] = False         # one repair, two losses
    pres[3, [1]] = False            # no repair present
    pres[4, [7]] = False            # its only repair is invalid
    rp = pack(np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 0, 1]], bool))
    s = m.solve(K, seed, off, nss, pack(pres), rp)
    assert s.status.tolist() == [RECOVERED, SINGULAR, NOTHING, NOTHING, NOTHING]
    assert np.nonzero(s.det[0])[0].tolist() == [1, 2]
    assert s.selected.tolist()[:2] == [[True, True, True], [False, False, True]]
    assert not s.det[1:].any()
    alone = m.windows_alone(s, off, nss)
    assert np.array_equal(alone, s.det)  # disjoint windows: the joint decode finds nothing more
