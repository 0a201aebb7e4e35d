"""Full-rank recovery above the packed decode -- the row forms, the block service, the protocol operations'
mode switch and the batcher's -- through the C ABI, without a GPU: the nine symbols, their declarations, the
Python mirrors and the argument checks that come before any device call."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID, ERR_NOMEM = 0, -1, -4

ENGINE = ("fecgpu_rlc_decode_rows_full", "fecgpu_rlc_decode_rows_fused_full", "fecgpu_rlc_decode_rows_host_full",
          "fecgpu_rlc_decode_rows_fused_host_full", "fecgpu_block_svc_rlc_decode_full")
PROTOOPS = ("pquic_fec_set_recover_mode", "pquic_fec_get_recover_mode", "pquic_fec_singular_blocks")
BATCH = ("pquic_fec_batch_set_full_rank",)
HEADERS = {"fecgpu.h": ENGINE, "pquic_fec_protoops.h": PROTOOPS, "pquic_fec_batch.h": BATCH}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from pquic_amd.engine import load_library
    return load_library(LIB, private=True)


def err(lib):
    return lib.fecgpu_last_error().decode()


def test_nine_symbols_exported_and_declared(lib):
    assert sum(len(v) for v in HEADERS.values()) == 9
    for header, names in HEADERS.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert hasattr(lib, name), name
            assert re.search(r"^(int|uint64_t)\s+%s\s*\(" % name, text, re.M), (header, name)


def test_python_methods_exist():
    from pquic_amd.engine import Engine, HostPath
    for cls in (Engine, HostPath):
        for m in ("rlc_decode_rows_full", "rlc_decode_rows_fused_full"):
            assert inspect.isfunction(getattr(cls, m, None)), (cls.__name__, m)


# a buffer that stands for every table: never read by a refused call
BUF = np.zeros(1 << 12, np.uint64)
P = BUF.ctypes.data


def _rows(lib, src_rows=P, rep_rows=P, nb=2, k=4, r=2, L=16, seed=P, sp=P, rp=P, st=P, rec=P, ws=P, wsb=1 << 15):
    return lib.fecgpu_rlc_decode_rows_full(src_rows, rep_rows, nb, k, r, L, seed, sp, rp, st, rec, ws, wsb, None)


def _fused(lib, src_rows=P, src_len=P, rep_rows=P, rep_len=P, blk_len=P, nb=2, k=4, r=2, L=16, seed=P, sp=P, rp=P,
           st=P, rec=P, ws=P, wsb=1 << 15):
    return lib.fecgpu_rlc_decode_rows_fused_full(src_rows, src_len, rep_rows, rep_len, blk_len, nb, k, r, L, seed, sp,
                                                 rp, st, rec, ws, wsb, None)


def test_device_row_forms_refuse_null_arguments(lib):
    for kw in ("src_rows", "rep_rows", "seed", "sp", "rp", "st", "rec", "ws"):
        assert _rows(lib, **{kw: None}) == ERR_INVALID, kw
    for kw in ("src_rows", "src_len", "rep_rows", "rep_len", "blk_len", "seed", "sp", "rp", "st", "rec", "ws"):
        assert _fused(lib, **{kw: None}) == ERR_INVALID, kw


@pytest.mark.parametrize("call", [_rows, _fused])
def test_device_row_forms_shape_workspace_and_empty_batch(lib, call):
    assert call(lib, k=129) == ERR_INVALID
    assert call(lib, k=0) == ERR_INVALID
    assert call(lib, r=129) == ERR_INVALID
    for L in (0, 6, 1201):
        assert call(lib, L=L) == ERR_INVALID, L
    need = lib.fecgpu_rlc_decode_workspace(2, 4, 2)
    assert need > 0
    assert call(lib, wsb=need - 1) == ERR_NOMEM
    assert call(lib, nb=0) == OK


def _tables(nb, k, r, blk, src):
    return dict(src_rows=np.zeros(nb * k, np.uint64), src_len=np.full(nb * k, src, np.uint32),
                rep_rows=np.zeros(nb * r, np.uint64), rep_len=np.full(nb * r, blk, np.uint32),
                blk_len=np.full(nb, blk, np.uint32), seeds=np.zeros(nb * r, np.uint32),
                sp=np.full(2 * nb, 0xF, np.uint64), rp=np.full(2 * nb, 0x3, np.uint64), st=np.full(nb, 0xEE, np.uint8),
                rec=np.full(2 * nb, 0x55, np.uint64))


ROWS_KEYS = ("src_rows", "rep_rows", "seeds", "sp", "rp", "st", "rec")
FUSED_KEYS = ("src_rows", "src_len", "rep_rows", "rep_len", "blk_len", "seeds", "sp", "rp", "st", "rec")


def _rows_host(lib, t, nb, k, r, L, drop=None):
    a = {x: (None if x == drop else t[x].ctypes.data) for x in ROWS_KEYS}
    return lib.fecgpu_rlc_decode_rows_host_full(None, a["src_rows"], a["rep_rows"], nb, k, r, L, a["seeds"], a["sp"],
                                                a["rp"], a["st"], a["rec"])


def _fused_host(lib, t, nb, k, r, L, drop=None):
    a = {x: (None if x == drop else t[x].ctypes.data) for x in FUSED_KEYS}
    return lib.fecgpu_rlc_decode_rows_fused_host_full(None, a["src_rows"], a["src_len"], a["rep_rows"], a["rep_len"],
                                                      a["blk_len"], nb, k, r, L, a["seeds"], a["sp"], a["rp"], a["st"],
                                                      a["rec"])


def test_host_row_forms_refuse_without_a_device(lib):
    """No context can exist without a device, so every call is refused and nothing is written; the fused
    form checks its tables, shape and lengths before it looks at the context, as its reference-mode twin."""
    nb, k, r, L = 3, 4, 2, 1200
    for key in ROWS_KEYS:
        t = _tables(nb, k, r, 1000, 1000)
        assert _rows_host(lib, t, nb, k, r, L, drop=key) == ERR_INVALID, key
        assert (t["st"] == 0xEE).all() and (t["rec"] == 0x55).all()
    t = _tables(nb, k, r, 1000, 1000)
    assert _rows_host(lib, t, nb, k, r, L) == ERR_INVALID      # no context
    assert _rows_host(lib, t, nb, 129, r, L) == ERR_INVALID
    assert _rows_host(lib, t, nb, k, 129, L) == ERR_INVALID
    assert _rows_host(lib, t, nb, k, r, 1202) == ERR_INVALID
    for key in FUSED_KEYS:
        t = _tables(nb, k, r, 1000, 1000)
        assert _fused_host(lib, t, nb, k, r, L, drop=key) == ERR_INVALID, key
        assert "NULL" in err(lib), key
    t = _tables(nb, k, r, 1000, 1000)
    assert _fused_host(lib, t, nb, k, r, L) == ERR_INVALID and "context" in err(lib)
    for name, val in dict(k=129, r=129, L=1202).items():
        args = dict(k=k, r=r, L=L)
        args[name] = val
        assert _fused_host(lib, _tables(nb, 129, 129, 8, 8), nb, args["k"], args["r"], args["L"]) == ERR_INVALID
        assert "context" not in err(lib), name
    t = _tables(nb, k, r, 1000, 1000)
    t["src_len"][nb * k - 1] = 1001
    assert _fused_host(lib, t, nb, k, r, L) == ERR_INVALID and "src_len" in err(lib)
    assert (t["st"] == 0xEE).all() and (t["rec"] == 0x55).all()


def test_block_service_full_refuses_null_service(lib):
    f = lib.fecgpu_block_svc_rlc_decode_full
    assert f(None, P, P, P, 16, 4, 1200, P, P, P, P, P) == ERR_INVALID


def test_recover_mode_switch(lib):
    set_mode, get_mode = lib.pquic_fec_set_recover_mode, lib.pquic_fec_get_recover_mode
    set_mode.argtypes = [C.c_int]
    lib.pquic_fec_singular_blocks.restype = C.c_uint64
    try:
        assert get_mode() == 0  # reference mode is the default
        assert set_mode(1) == 0 and get_mode() == 1
        for bad in (2, -1):
            assert set_mode(bad) == -1 and get_mode() == 1
        assert set_mode(0) == 0 and get_mode() == 0
        for bad in (2, -1):
            assert set_mode(bad) == -1 and get_mode() == 0
        before = lib.pquic_fec_singular_blocks()
        assert lib.pquic_fec_singular_blocks() == before  # reading the counter does not move it
    finally:
        set_mode(0)


def test_batcher_full_rank_refuses_null(lib):
    f = lib.pquic_fec_batch_set_full_rank
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(None, 1) == -1
