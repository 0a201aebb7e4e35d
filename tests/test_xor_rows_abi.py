"""The XOR row entry points through the C ABI, without a GPU: the four symbols, their Python mirrors and
the argument checks that come before any launch.  No device call is made: every refused call returns
before it touches HIP, and the host forms check their tables and lengths before they look at the
context."""
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID = 0, -1

SYMBOLS = ("fecgpu_xor_encode_rows", "fecgpu_xor_decode_rows", "fecgpu_xor_encode_rows_host",
           "fecgpu_xor_decode_rows_host")


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
    for cls in (Engine, HostPath):
        for m in ("xor_encode_rows", "xor_decode_rows"):
            assert inspect.isfunction(getattr(cls, m, None)), (cls.__name__, m)


# a buffer that stands for every table: never read by a refused call
BUF = np.zeros(1 << 12, np.uint64)
P = BUF.ctypes.data


def _encode(lib, src_rows=P, src_len=P, rep_rows=P, blk_len=P, nb=2, k=4, L=16):
    return lib.fecgpu_xor_encode_rows(src_rows, src_len, rep_rows, blk_len, nb, k, L, None)


def _decode(lib, src_rows=P, src_len=P, rep_rows=P, blk_len=P, nb=2, k=4, L=16, sp=P, rp=P, st=P, rec=P):
    return lib.fecgpu_xor_decode_rows(src_rows, src_len, rep_rows, blk_len, nb, k, L, sp, rp, st, rec, None)


def test_null_tables_are_refused(lib):
    for kw in ("src_rows", "src_len", "rep_rows", "blk_len"):
        assert _encode(lib, **{kw: None}) == ERR_INVALID, kw
    for kw in ("src_rows", "src_len", "rep_rows", "blk_len", "sp", "rp", "st", "rec"):
        assert _decode(lib, **{kw: None}) == ERR_INVALID, kw


def test_shape_limits_are_refused(lib):
    for call in (_encode, _decode):
        assert call(lib, k=0) == ERR_INVALID
        assert call(lib, k=129) == ERR_INVALID
        for L in (0, 6, 1201, 65536):
            assert call(lib, L=L) == ERR_INVALID, L


def test_empty_batches_are_accepted_without_a_launch(lib):
    assert _encode(lib, nb=0) == OK
    assert _decode(lib, nb=0) == OK
    assert _encode(lib, nb=0, k=128, L=65532) == OK  # the limits themselves
    assert _decode(lib, nb=0, k=1, L=4) == OK


def _host_tables(nb, k, blk, src):
    return dict(src_rows=np.zeros(nb * k, np.uint64), src_len=np.full(nb * k, src, np.uint32),
                rep_rows=np.zeros(nb, np.uint64), blk_len=np.full(nb, blk, np.uint32),
                sp=np.full(2 * nb, (1 << k) - 2 if k < 64 else 2 ** 64 - 2, np.uint64),
                rp=np.full(2 * nb, 1, np.uint64), st=np.zeros(nb, np.uint8), rec=np.zeros(2 * nb, np.uint64))


def _enc_host(lib, t, nb, k, L, ctx=None):
    return lib.fecgpu_xor_encode_rows_host(ctx, t["src_rows"].ctypes.data, t["src_len"].ctypes.data,
                                           t["rep_rows"].ctypes.data, t["blk_len"].ctypes.data, nb, k, L)


def _dec_host(lib, t, nb, k, L, ctx=None):
    return lib.fecgpu_xor_decode_rows_host(ctx, t["src_rows"].ctypes.data, t["src_len"].ctypes.data,
                                           t["rep_rows"].ctypes.data, t["blk_len"].ctypes.data, nb, k, L,
                                           t["sp"].ctypes.data, t["rp"].ctypes.data, t["st"].ctypes.data,
                                           t["rec"].ctypes.data)


@pytest.mark.parametrize("host", [_enc_host, _dec_host])
def test_host_forms_refuse_length_violations(lib, host):
    """src_len <= blk_len <= symbol_size is checked on the host tables before the context is looked at, so
    the refusal is visible without a device: the message names the rule that failed."""
    nb, k, L = 3, 4, 1200
    t = _host_tables(nb, k, blk=1000, src=1000)
    assert host(lib, t, nb, k, L) == ERR_INVALID and "context" in err(lib)  # lengths fine: only no context
    t = _host_tables(nb, k, blk=1000, src=1000)
    t["src_len"][nb * k - 1] = 1001  # the last block's last source: present in both forms' tables
    assert host(lib, t, nb, k, L) == ERR_INVALID and "src_len" in err(lib)
    t = _host_tables(nb, k, blk=1000, src=0)
    t["blk_len"][1] = 1204
    assert host(lib, t, nb, k, L) == ERR_INVALID and "blk_len" in err(lib)
    t = _host_tables(nb, k, blk=1200, src=1200)  # the limits themselves are accepted
    assert host(lib, t, nb, k, L) == ERR_INVALID and "context" in err(lib)
    t = _host_tables(nb, 128, blk=65532, src=65532)
    assert host(lib, t, nb, 128, 65532) == ERR_INVALID and "context" in err(lib)
    t = _host_tables(nb, 1, blk=4, src=4)
    t["sp"][:] = 1
    assert host(lib, t, nb, 1, 4) == ERR_INVALID and "context" in err(lib)
    for kk, LL in ((0, L), (129, L), (k, 0), (k, 6), (k, 1201), (k, 65536)):
        assert host(lib, _host_tables(nb, 129, 4, 4), nb, kk, LL) == ERR_INVALID
        assert "context" not in err(lib), (kk, LL)


@pytest.mark.parametrize("host", [_enc_host, _dec_host])
def test_host_forms_refuse_null_tables(lib, host):
    nb, k, L = 2, 4, 16
    t = _host_tables(nb, k, blk=16, src=16)
    names = ("src_rows", "src_len", "rep_rows", "blk_len") + (("sp", "rp", "st", "rec") if host is _dec_host else ())

    class Null:  # stands for a NULL table
        class ctypes:
            data = None
    for name in names:
        bad = dict(t)
        bad[name] = Null
        assert host(lib, bad, nb, k, L) == ERR_INVALID and "NULL" in err(lib) and "context" not in err(lib), name


def test_decode_host_ignores_the_length_of_an_absent_source(lib):
    nb, k, L = 2, 4, 1200
    t = _host_tables(nb, k, blk=800, src=800)
    t["sp"][:] = 0
    t["sp"][0] = 0b1011
    t["sp"][2] = 0b1111
    t["src_len"][2] = 5000  # block 0, source 2: absent, its length entry is not looked at
    assert _dec_host(lib, t, nb, k, L) == ERR_INVALID and "context" in err(lib)
    t["src_len"][4 + 2] = 5000  # block 1, source 2: present
    assert _dec_host(lib, t, nb, k, L) == ERR_INVALID and "src_len" in err(lib)
    t["src_len"][4 + 2] = 800
    t["sp"][1] = 2 ** 64 - 1  # mask bits above k name no source: their length entries do not exist
    assert _dec_host(lib, t, nb, k, L) == ERR_INVALID and "context" in err(lib)
