"""The block service's row requests and the hooks' in-place switch through the C ABI, without a GPU: the
symbols, their declarations, their Python argument mirrors, and what the calls answer before they touch
a device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
ERR_INVALID = -1

SVC_SYMBOLS = ("fecgpu_block_svc_rlc_encode_rows", "fecgpu_block_svc_rlc_decode_rows",
               "fecgpu_block_svc_xor_encode_rows", "fecgpu_block_svc_xor_decode_rows")
HOOK_SYMBOLS = ("pquic_fec_set_hooks_in_place", "pquic_fec_get_hooks_in_place", "pquic_fec_register_heap",
                "pquic_fec_unregister_heap", "pquic_fec_hook_rows_stats")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from pquic_amd.engine import load_library
    return load_library(LIB, private=True)


def test_row_requests_are_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    for name in SVC_SYMBOLS:
        assert hasattr(lib, name), name
        assert "int " + name + "(fecgpu_block_svc_t *svc, const uint64_t *src_rows, const uint32_t *src_len," in text, name
        assert getattr(lib, name).argtypes is not None, name  # mirrored in pquic_amd/engine.py


def test_hook_switch_is_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "pquic_fec_protoops.h")).read()
    for name in HOOK_SYMBOLS:
        assert hasattr(lib, name), name
        assert name + "(" in text, name
    assert "pquic_fec_protoop_stats_t" in text
    # the counters are a function of their own: the stats struct keeps its six words
    stats = text[text.index("typedef struct {\n    uint64_t generate_calls"):text.index("} pquic_fec_protoop_stats_t;")]
    assert stats.count("uint64_t") == 2 and "svc_deadline_misses" in stats


def test_a_missing_service_is_refused_before_any_table_is_read(lib):
    """No service (NULL): FECGPU_ERR_INVALID, the answer a caller takes the launch path on; the tables are
    not looked at (they are NULL here)."""
    assert lib.fecgpu_block_svc_rlc_encode_rows(None, None, None, None, 1200, 16, 4, 7) == ERR_INVALID
    assert lib.fecgpu_block_svc_rlc_decode_rows(None, None, None, None, None, 1200, 16, 4, None, None, None, 0, None,
                                                None) == ERR_INVALID
    assert lib.fecgpu_block_svc_xor_encode_rows(None, None, None, 0, 1200, 4) == ERR_INVALID
    assert lib.fecgpu_block_svc_xor_decode_rows(None, None, None, 0, 1200, 4, None, None, None, None) == ERR_INVALID


def test_switch_defaults_to_staged_and_takes_only_0_and_1(lib):
    assert lib.pquic_fec_get_hooks_in_place() == 0
    for bad in (-1, 2, 100):
        assert lib.pquic_fec_set_hooks_in_place(bad) == -1
        assert lib.pquic_fec_get_hooks_in_place() == 0
    try:
        assert lib.pquic_fec_set_hooks_in_place(1) == 0  # this library has the row requests
        assert lib.pquic_fec_get_hooks_in_place() == 1
    finally:
        assert lib.pquic_fec_set_hooks_in_place(0) == 0
    assert lib.pquic_fec_get_hooks_in_place() == 0


def test_counters_start_at_zero_and_bad_heaps_are_refused(lib):
    out = np.full(4, 99, np.uint64)
    lib.pquic_fec_hook_rows_stats.argtypes = [C.c_void_p]
    lib.pquic_fec_hook_rows_stats.restype = None
    lib.pquic_fec_hook_rows_stats(out.ctypes.data)
    assert out.tolist() == [0, 0, 0, 0]
    lib.pquic_fec_register_heap.argtypes = [C.c_void_p, C.c_size_t]
    lib.pquic_fec_unregister_heap.argtypes = [C.c_void_p]
    assert lib.pquic_fec_register_heap(None, 4096) == -1
    assert lib.pquic_fec_register_heap(out.ctypes.data, 0) == -1
    assert lib.pquic_fec_unregister_heap(None) == -1
