"""C-ABI boundary of the full-rank decode mode, without a GPU: the entry points exist, the header
defines the new status, and arguments are validated before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")

v, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
OK, ERR_INVALID, ERR_NOMEM = 0, -1, -4


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = C.CDLL(LIB)
    L.fecgpu_rlc_decode_workspace.restype = sz
    L.fecgpu_rlc_decode_workspace.argtypes = [u64, u32, u32]
    return L


def test_symbols_exported(lib):
    for name in ("fecgpu_rlc_decode_plan_full", "fecgpu_rlc_decode_full", "fecgpu_rlc_decode_host_full"):
        assert hasattr(lib, name), name


def test_header_defines_singular():
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    assert re.search(r"^#define\s+FECGPU_BLOCK_SINGULAR\s+3\b", text, re.M)
    for name in ("fecgpu_rlc_decode_plan_full", "fecgpu_rlc_decode_full", "fecgpu_rlc_decode_host_full"):
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name


def test_decode_full_argument_validation_without_device(lib):
    f = lib.fecgpu_rlc_decode_full
    f.argtypes = [v, v, u64, u32, u32, u32, u32, v, v, v, v, v, v, v, sz, v]
    big = 1 << 30
    # src, rep, nblocks, k, r, L, fbn_base, fbn, rep_seed, sp, rp, status, recovered, ws, wsb, stream
    assert f(None, None, 0, 16, 4, 1200, 0, None, None, None, None, None, None, None, 0, None) == OK  # empty
    assert f(None, None, 1, 16, 4, 1200, 0, None, None, 16, 16, 16, 16, 16, big, None) == ERR_INVALID  # NULL rows
    assert f(16, 16, 1, 16, 4, 1200, 0, None, None, None, 16, 16, 16, 16, big, None) == ERR_INVALID   # NULL mask
    assert f(16, 16, 1, 16, 4, 1200, 0, None, None, 16, 16, None, 16, 16, big, None) == ERR_INVALID   # NULL status
    assert f(16, 16, 1, 16, 4, 1200, 0, None, None, 16, 16, 16, 16, None, big, None) == ERR_INVALID   # NULL ws
    assert f(16, 16, 1, 16, 4, 1201, 0, None, None, 16, 16, 16, 16, 16, big, None) == ERR_INVALID     # L % 4
    assert f(16, 16, 1, 129, 4, 1200, 0, None, None, 16, 16, 16, 16, 16, big, None) == ERR_INVALID    # k > 128
    assert f(16, 16, 1, 16, 129, 1200, 0, None, None, 16, 16, 16, 16, 16, big, None) == ERR_INVALID   # r > 128
    need = lib.fecgpu_rlc_decode_workspace(8, 16, 4)
    assert f(16, 16, 8, 16, 4, 1200, 0, None, None, 16, 16, 16, 16, 16, need - 1, None) == ERR_NOMEM


def test_plan_full_argument_validation_without_device(lib):
    f = lib.fecgpu_rlc_decode_plan_full
    f.argtypes = [u64, u32, u32, u32, v, v, v, v, v, sz, v]
    big = 1 << 30
    # nblocks, k, r, fbn_base, fbn, rep_seed, sp, rp, ws, wsb, stream
    assert f(0, 16, 4, 0, None, None, None, None, None, 0, None) == OK
    assert f(1, 16, 4, 0, None, None, None, 16, 16, big, None) == ERR_INVALID
    assert f(1, 16, 4, 0, None, None, 16, None, 16, big, None) == ERR_INVALID
    assert f(1, 16, 4, 0, None, None, 16, 16, None, big, None) == ERR_INVALID
    assert f(1, 129, 4, 0, None, None, 16, 16, 16, big, None) == ERR_INVALID
    assert f(1, 0, 4, 0, None, None, 16, 16, 16, big, None) == ERR_INVALID
    need = lib.fecgpu_rlc_decode_workspace(8, 16, 4)
    assert f(8, 16, 4, 0, None, None, 16, 16, 16, need - 1, None) == ERR_NOMEM


def test_host_full_argument_validation_without_device(lib):
    f = lib.fecgpu_rlc_decode_host_full
    f.argtypes = [v, v, v, u64, u32, u32, u32, u32, v, v, v, v, v, v]
    # ctx, src, rep, nblocks, k, r, L, fbn_base, fbn, rep_seed, sp, rp, status, recovered
    assert f(None, 16, 16, 1, 16, 4, 1200, 0, None, None, 16, 16, 16, 16) == ERR_INVALID  # no context
    assert f(None, None, None, 0, 16, 4, 1200, 0, None, None, None, None, None, None) == ERR_INVALID


def test_package_exports_block_constants():
    import pquic_amd
    assert (pquic_amd.BLOCK_RECOVERED, pquic_amd.BLOCK_NOTHING, pquic_amd.BLOCK_REF_UB,
            pquic_amd.BLOCK_SINGULAR) == (0, 1, 2, 3)
    for name in ("BLOCK_RECOVERED", "BLOCK_NOTHING", "BLOCK_REF_UB", "BLOCK_SINGULAR"):
        assert name in pquic_amd.__all__
    for name in ("rlc_decode_full", "rlc_decode_plan_full"):
        assert hasattr(pquic_amd.Engine, name)
    assert hasattr(pquic_amd.HostPath, "rlc_decode_full")
