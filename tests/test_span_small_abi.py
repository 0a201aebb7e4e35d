"""The one-launch span decode's counter and the blocking span recovery call through the C ABI, without a GPU:
the exported symbols and their declarations, the Python mirror, the counter at rest, and every refusal of
pquic_fec_rlc_recover_span that comes before the engine is touched.  No device call is made."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
DRIVER = os.path.join(ROOT, "tools", "libspanload.so")
ERR_UNBOUND = 0x41B


class Span(C.Structure):  # pquic_fec_span_t
    _fields_ = [("base_id", C.c_uint32), ("K", C.c_uint32), ("R", C.c_uint32), ("src", C.c_void_p),
                ("rep", C.c_void_p), ("first_id", C.c_void_p), ("nss", C.c_void_p)]


class Repair(C.Structure):  # pquic_repair_symbol_t
    _fields_ = [("fpid", C.c_uint64), ("data_length", C.c_uint16), ("data", C.c_void_p)]


GET = C.CFUNCTYPE(C.c_uint64, C.c_void_p, C.c_uint16, C.c_uint16)
SET = C.CFUNCTYPE(None, C.c_void_p, C.c_uint16, C.c_uint16, C.c_uint64)
MALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint)
FREE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


class HostApi(C.Structure):  # pquic_fec_host_api_t
    _fields_ = [("get_cnx", GET), ("set_cnx", SET), ("my_malloc", MALLOC), ("my_free", FREE), ("skip_frame", C.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = C.CDLL(LIB)
    L.fecgpu_rlc_span_one_launch_calls.restype = C.c_uint64
    L.fecgpu_rlc_span_one_launch_calls.argtypes = []
    L.pquic_fec_rlc_recover_span.restype = C.c_uint64
    L.pquic_fec_rlc_recover_span.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pquic_fec_bind_host.argtypes = [C.c_void_p, C.c_int]
    return L


def test_symbols_are_exported_and_declared(lib):
    assert hasattr(lib, "fecgpu_rlc_span_one_launch_calls") and hasattr(lib, "pquic_fec_rlc_recover_span")
    engine_h = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    assert "uint64_t fecgpu_rlc_span_one_launch_calls(void);" in engine_h
    hooks_h = open(os.path.join(ROOT, "include", "pquic_fec_protoops.h")).read()
    assert "protoop_arg_t pquic_fec_rlc_recover_span(picoquic_cnx_t *cnx, const pquic_fec_span_t *sp," in hooks_h
    assert "} pquic_fec_span_t;" in hooks_h  # the span's type moved here; the batch header includes this one
    # no symbol can be longer than 32767 bytes, so the call has no such refusal to make: the length has 15 bits
    assert hooks_h.count("uint16_t data_length : 15;") == 2
    batch_h = open(os.path.join(ROOT, "include", "pquic_fec_batch.h")).read()
    assert "} pquic_fec_span_t;" not in batch_h and '#include "pquic_fec_protoops.h"' in batch_h


def test_python_mirror_and_counter_at_rest(lib):
    import pquic_amd
    # process-wide, so 0 only where no span decode has run: a fresh process that loads the library and reads it
    code = ("import ctypes as C; L = C.CDLL(%r); f = L.fecgpu_rlc_span_one_launch_calls; f.restype = C.c_uint64; "
            "print(f(), f())" % LIB)
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.split() == \
        ["0", "0"]
    before = lib.fecgpu_rlc_span_one_launch_calls()
    assert pquic_amd.span_one_launch_calls() == before  # the mirror reads the same counter; reading does not move it
    assert hasattr(pquic_amd.Engine, "span_one_launch_calls")
    assert lib.fecgpu_rlc_span_one_launch_calls() == before


def test_driver_exports():
    assert os.path.exists(DRIVER), "run __graft_entry__.build() first"
    d = C.CDLL(DRIVER)
    for name in ("sl_recover_span", "sl_run_blocking", "sl_ticket", "sl_ticket_cols", "sl_submit", "sl_run"):
        assert hasattr(d, name), name


def span_1x1(keep, **over):
    """a well-formed span of one missing column under one repair of 4 bytes"""
    data = (C.c_uint8 * 4)(1, 2, 3, 4)
    rep = Repair(0, 4, C.addressof(data))
    src = (C.c_void_p * 1)(None)
    reps = (C.c_void_p * 1)(C.addressof(rep))
    first = (C.c_uint32 * 1)(7)
    nss = (C.c_uint8 * 1)(1)
    sp = Span(7, 1, 1, C.addressof(src), C.addressof(reps), C.addressof(first), C.addressof(nss))
    for k, v in over.items():
        if k == "nss0":
            nss[0] = v
        elif k == "first0":
            first[0] = v
        elif k == "rep0":
            reps[0] = v
        else:
            setattr(sp, k, v)
    keep.extend([data, rep, src, reps, first, nss, sp])
    return sp


def call(lib, sp, rec=True, nrec=True):
    out = (C.c_void_p * 128)(*([0x1] * 128))
    n = C.c_uint32(77)
    ret = lib.pquic_fec_rlc_recover_span(None, C.byref(sp) if sp is not None else None, out if rec else None,
                                         C.byref(n) if nrec else None)
    return ret, n.value


def test_refused_before_binding(lib):
    lib.pquic_fec_bind_host(None, 0)
    keep = []
    assert call(lib, span_1x1(keep)) == (ERR_UNBOUND, 0)
    assert call(lib, None) == (ERR_UNBOUND, 0)


def test_refusals_when_bound_allocate_nothing(lib):
    mallocs = []
    before = lib.fecgpu_rlc_span_one_launch_calls()

    def my_malloc(cnx, n):
        mallocs.append(n)
        return None

    api = HostApi(GET(lambda c, a, p: 0), SET(lambda c, a, p, v: None), MALLOC(my_malloc), FREE(lambda c, p: None), None)
    assert lib.pquic_fec_bind_host(C.byref(api), 0) == 0
    try:
        keep = []
        assert call(lib, None) == (ERR_UNBOUND, 0)                      # NULL span
        assert call(lib, span_1x1(keep), rec=False) == (ERR_UNBOUND, 0)  # NULL recovered[]
        assert call(lib, span_1x1(keep), nrec=False)[0] == ERR_UNBOUND   # NULL nrecovered
        for over in (dict(K=0), dict(K=129), dict(R=0), dict(R=129), dict(src=None), dict(rep=None),
                     dict(first_id=None), dict(nss=None), dict(rep0=None), dict(nss0=0), dict(nss0=2),
                     dict(first0=8), dict(first0=6)):  # (base_id 7, K 1: offsets 1 and 2^32 - 1 leave the span)
            assert call(lib, span_1x1(keep, **over)) == (ERR_UNBOUND, 0), over
        assert mallocs == []
    finally:
        lib.pquic_fec_bind_host(None, 0)
    assert lib.fecgpu_rlc_span_one_launch_calls() == before
