"""The span_compact knob and the batching adapter's span entry point through the C ABI, without a GPU: the
knob's default and range, the exported symbol, and the stats struct's layout as the span driver
(tools/libspanload.so) reports it.  No device call is made."""
import ctypes as C
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
DRIVER = os.path.join(ROOT, "tools", "libspanload.so")
OK, ERR_INVALID = 0, -1


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = C.CDLL(LIB)
    L.fecgpu_set_knob.argtypes = [C.c_char_p, C.c_int]
    L.fecgpu_get_knob.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    return L


@pytest.fixture(scope="module")
def driver():
    assert os.path.exists(DRIVER), "run __graft_entry__.build() first"
    return C.CDLL(DRIVER)


def get(lib, name):
    v = C.c_int(-12345)
    return lib.fecgpu_get_knob(name, C.byref(v)), v.value


def test_knob_default_and_range(lib):
    assert get(lib, b"span_compact") == (OK, 1)
    try:
        assert lib.fecgpu_set_knob(b"span_compact", 0) == OK
        assert get(lib, b"span_compact") == (OK, 0)
        for bad in (2, -1):
            assert lib.fecgpu_set_knob(b"span_compact", bad) == ERR_INVALID
            assert get(lib, b"span_compact") == (OK, 0)  # a refused value changes nothing
    finally:
        assert lib.fecgpu_set_knob(b"span_compact", 1) == OK
    assert get(lib, b"span_compact") == (OK, 1)


def test_header_documents_the_knob():
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    assert '"span_compact"' in text


def test_span_entry_point_is_exported(lib):
    fn = lib.pquic_fec_batch_recover_span
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn(None, None, None, 0, None, None) == -1  # no batcher, no span: refused before anything is touched


def test_stats_keep_the_old_fields_first(driver):
    off = (C.c_int * 10)()
    size = driver.sl_stats_layout(off)
    # submitted, completed, batches, immediate, engine_errors, rows_in_place, rows_staged, deadline_holds: where
    # they were; spans and span_symbols appended
    assert list(off) == [0, 8, 16, 48, 56, 104, 112, 136, 144, 152]
    assert size == 160


def test_driver_exports(driver):
    for name in ("sl_open", "sl_close", "sl_live", "sl_source", "sl_repair", "sl_submit", "sl_poll", "sl_drain",
                 "sl_ticket", "sl_ticket_cols", "sl_release", "sl_stats", "sl_run"):
        assert hasattr(driver, name), name
