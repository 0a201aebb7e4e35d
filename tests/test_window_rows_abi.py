"""The window-rows entry points through the C ABI, without a GPU: the three symbols, their Python mirrors
and the argument checks that come before any launch.  No device call is made: every refused call returns
before it touches HIP, and the host form checks its tables before it looks at the context."""
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID = 0, -1

SYMBOLS = ("fecgpu_rlc_window_rows_workspace", "fecgpu_rlc_window_encode_rows",
           "fecgpu_rlc_window_encode_rows_host")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from pquic_amd.engine import load_library
    return load_library(LIB, private=True)


def err(lib):
    return lib.fecgpu_last_error().decode()


def test_symbols_are_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    for name in SYMBOLS:
        assert name + "(" in text, name


def test_engine_has_the_methods():
    from pquic_amd.engine import Engine, HostPath
    for m in ("rlc_window_encode_rows", "window_rows_workspace_bytes", "rlc_window_encode_table"):
        assert inspect.isfunction(getattr(Engine, m, None)), m
    assert inspect.isfunction(getattr(HostPath, "rlc_window_encode_rows", None))


def test_workspace_is_the_stream_at_the_width(lib):
    """nrows rows of symbol_size rounded up to 16"""
    assert lib.fecgpu_rlc_window_rows_workspace(0, 1200) == 0
    assert lib.fecgpu_rlc_window_rows_workspace(7, 1200) == 7 * 1200
    assert lib.fecgpu_rlc_window_rows_workspace(7, 1500) == 7 * 1504
    assert lib.fecgpu_rlc_window_rows_workspace(3, 4) == 3 * 16


# a buffer that stands for every table and the workspace: never read by a refused call
BUF = np.zeros(1 << 12, np.uint64)
P = BUF.ctypes.data + (-BUF.ctypes.data) % 16


def _dev(lib, rows=P, row_len=P, nrows=8, wrow=P, rep_rows=P, blk_len=P, nwin=2, k=4, r=2, L=16, ws=P, wsb=1 << 12):
    return lib.fecgpu_rlc_window_encode_rows(rows, row_len, nrows, wrow, rep_rows, blk_len, nwin, k, r, L, ws, wsb,
                                             None)


def test_device_form_refuses_null_tables(lib):
    for kw in ("rows", "row_len", "wrow", "rep_rows", "blk_len", "ws"):
        assert _dev(lib, **{kw: None}) == ERR_INVALID, kw


def test_device_form_refuses_shape_limits(lib):
    assert _dev(lib, k=0) == ERR_INVALID
    assert _dev(lib, k=129, nrows=200) == ERR_INVALID
    assert _dev(lib, r=0) == ERR_INVALID
    assert _dev(lib, r=129) == ERR_INVALID
    for L in (0, 6, 1201, 65536):
        assert _dev(lib, L=L) == ERR_INVALID, L
    assert _dev(lib, nrows=3) == ERR_INVALID and "shorter" in err(lib)  # a stream of fewer than k rows
    assert _dev(lib, ws=P + 4) == ERR_INVALID and "aligned" in err(lib)
    # (nrows + k) * width at 2 GiB: the rule of the 32-bit load offsets, named
    assert _dev(lib, nrows=(1 << 31) // 1200, L=1200, wsb=1 << 40) == ERR_INVALID and "2 GiB" in err(lib)
    assert _dev(lib, wsb=8 * 16 - 1) != OK and "workspace" in err(lib)


def test_empty_calls_are_accepted_without_a_launch(lib):
    assert _dev(lib, nwin=0) == OK
    assert _dev(lib, nwin=0, k=128, r=128, L=65532) == OK
    t = _host_tables(8, [], 4, 2, 16, 16)
    assert _host(lib, t, 8, 0, 4, 2, 16, ctx=1) == OK  # no window: the context is not dereferenced


def _host_tables(nrows, wrow, k, r, row, blk):
    nwin = len(wrow)
    return dict(rows=np.zeros(max(nrows, 1), np.uint64), row_len=np.full(max(nrows, 1), row, np.uint32),
                wrow=np.array(list(wrow) + [0], np.uint32), rep_rows=np.zeros(nwin * r + 1, np.uint64),
                blk_len=np.full(nwin + 1, blk, np.uint32))


def _host(lib, t, nrows, nwin, k, r, L, ctx=None):
    return lib.fecgpu_rlc_window_encode_rows_host(ctx, t["rows"].ctypes.data, t["row_len"].ctypes.data, nrows,
                                                  t["wrow"].ctypes.data, t["rep_rows"].ctypes.data,
                                                  t["blk_len"].ctypes.data, nwin, k, r, L)


def test_host_form_names_the_failed_rule(lib):
    """wrow[w] + k <= nrows, row_len <= symbol_size and blk_len <= symbol_size are checked on the host tables
    before the context is looked at, so the refusal is visible without a device."""
    nrows, k, r, L = 12, 4, 2, 1200
    wrow = [0, 1, 8, 8, 3]
    t = _host_tables(nrows, wrow, k, r, 1000, 1000)
    assert _host(lib, t, nrows, len(wrow), k, r, L) == ERR_INVALID and "context" in err(lib)  # only no context
    t["wrow"][2] = 9  # 9 + 4 > 12
    assert _host(lib, t, nrows, len(wrow), k, r, L) == ERR_INVALID and "wrow" in err(lib)
    t = _host_tables(nrows, wrow, k, r, 1000, 1000)
    t["row_len"][nrows - 1] = 1201
    assert _host(lib, t, nrows, len(wrow), k, r, L) == ERR_INVALID and "row_len" in err(lib)
    t = _host_tables(nrows, wrow, k, r, 1000, 1000)
    t["blk_len"][4] = 1204
    assert _host(lib, t, nrows, len(wrow), k, r, L) == ERR_INVALID and "blk_len" in err(lib)
    # the limits themselves, and a row longer than a window's length (truncated for that window, not refused)
    t = _host_tables(nrows, wrow, k, r, 1200, 1200)
    t["blk_len"][1] = 7
    assert _host(lib, t, nrows, len(wrow), k, r, L) == ERR_INVALID and "context" in err(lib)
    for kk, rr, LL in ((0, r, L), (129, r, L), (k, 0, L), (k, 129, L), (k, r, 0), (k, r, 6), (k, r, 1201), (k, r, 65536)):
        assert _host(lib, _host_tables(200, [0], 129, 2, 4, 4), 200, 1, kk, rr, LL) == ERR_INVALID
        assert "context" not in err(lib), (kk, rr, LL)


def test_host_form_refuses_null_tables(lib):
    nrows, k, r, L = 8, 4, 2, 16
    t = _host_tables(nrows, [0, 4], k, r, 16, 16)

    class Null:  # stands for a NULL table
        class ctypes:
            data = None
    for name in ("rows", "row_len", "wrow", "rep_rows", "blk_len"):
        bad = dict(t)
        bad[name] = Null
        assert _host(lib, bad, nrows, 2, k, r, L) == ERR_INVALID and "NULL" in err(lib) and "context" not in err(lib), name
