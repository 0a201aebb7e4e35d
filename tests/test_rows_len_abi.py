"""The ragged-row entry points through the C ABI, without a GPU: the seven symbols, their Python
mirrors, the argument checks that come before any launch, and the workspace function.  No device call
is made: every refused call returns before it touches HIP, and the host forms check their tables and
lengths before they look at the context."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID = 0, -1

SYMBOLS = ("fecgpu_rows_gather", "fecgpu_rows_scatter", "fecgpu_rlc_rows_len_workspace",
           "fecgpu_rlc_encode_rows_len", "fecgpu_rlc_decode_rows_len", "fecgpu_rlc_encode_rows_len_host",
           "fecgpu_rlc_decode_rows_len_host")


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
    for m in ("rows_gather", "rows_scatter", "rows_len_workspace_bytes", "rlc_encode_rows_len",
              "rlc_decode_rows_len"):
        assert inspect.isfunction(getattr(Engine, m, None)), m
    for m in ("rlc_encode_rows_len", "rlc_decode_rows_len"):
        assert inspect.isfunction(getattr(HostPath, m, None)), m


# a buffer that stands for every table: never read by a refused call
BUF = np.zeros(1 << 12, np.uint64)
P = BUF.ctypes.data


def _gather(lib, rows=P, lens=P, n=4, L=16, dst=P):
    return lib.fecgpu_rows_gather(rows, lens, n, L, dst, None)


def _scatter(lib, src=P, rows=P, lens=P, n=4, L=16):
    return lib.fecgpu_rows_scatter(src, rows, lens, n, L, None)


def _encode(lib, src_rows=P, src_len=P, rep_rows=P, blk_len=P, nb=2, k=4, r=2, L=16, ws=P, wsb=1 << 15):
    return lib.fecgpu_rlc_encode_rows_len(src_rows, src_len, rep_rows, blk_len, nb, k, r, L, 0, None, ws, wsb, None)


def _decode(lib, src_rows=P, src_len=P, rep_rows=P, rep_len=P, blk_len=P, nb=2, k=4, r=2, L=16, seed=P, sp=P, rp=P,
            st=P, rec=P, ws=P, wsb=1 << 15):
    return lib.fecgpu_rlc_decode_rows_len(src_rows, src_len, rep_rows, rep_len, blk_len, nb, k, r, L, seed, sp, rp,
                                          st, rec, ws, wsb, None)


def test_null_tables_are_refused(lib):
    assert _gather(lib, rows=None) == ERR_INVALID
    assert _gather(lib, lens=None) == ERR_INVALID
    assert _gather(lib, dst=None) == ERR_INVALID
    assert _scatter(lib, src=None) == ERR_INVALID
    assert _scatter(lib, rows=None) == ERR_INVALID
    assert _scatter(lib, lens=None) == ERR_INVALID
    for kw in ("src_rows", "src_len", "rep_rows", "blk_len", "ws"):
        assert _encode(lib, **{kw: None}) == ERR_INVALID, kw
    for kw in ("src_rows", "src_len", "rep_rows", "rep_len", "blk_len", "seed", "sp", "rp", "st", "rec", "ws"):
        assert _decode(lib, **{kw: None}) == ERR_INVALID, kw


def test_shape_limits_are_refused(lib):
    for call in (_encode, _decode):
        assert call(lib, k=129) == ERR_INVALID
        assert call(lib, k=0) == ERR_INVALID
        assert call(lib, r=129) == ERR_INVALID
        for L in (0, 6, 1201, 65536):
            assert call(lib, L=L) == ERR_INVALID, L
    for L in (0, 6, 1201, 65536):
        assert _gather(lib, L=L) == ERR_INVALID
        assert _scatter(lib, L=L) == ERR_INVALID
    assert _gather(lib, dst=P + 2) == ERR_INVALID  # the packed buffer is 4-byte aligned
    assert _scatter(lib, src=P + 2) == ERR_INVALID


def test_empty_batches_are_accepted_without_a_launch(lib):
    assert _gather(lib, n=0) == OK
    assert _scatter(lib, n=0) == OK
    assert _encode(lib, nb=0) == OK
    assert _decode(lib, nb=0) == OK


def test_workspace_too_small_is_refused(lib):
    need = lib.fecgpu_rlc_rows_len_workspace(2, 4, 2, 16)
    assert _decode(lib, wsb=need - 1) == -4  # FECGPU_ERR_NOMEM
    assert _encode(lib, wsb=2 * 4 * 16) == -4  # the packed sources alone


def _host_tables(nb, k, r, L, blk, src):
    return dict(src_rows=np.zeros(nb * k, np.uint64), src_len=np.full(nb * k, src, np.uint32),
                rep_rows=np.zeros(nb * r, np.uint64), rep_len=np.full(nb * r, blk, np.uint32),
                blk_len=np.full(nb, blk, np.uint32), seeds=np.zeros(nb * r, np.uint32),
                sp=np.full(2 * nb, 0xF, np.uint64), rp=np.full(2 * nb, 0x3, np.uint64), st=np.zeros(nb, np.uint8),
                rec=np.zeros(2 * nb, np.uint64))


def _enc_host(lib, t, nb, k, r, L, ctx=None):
    return lib.fecgpu_rlc_encode_rows_len_host(ctx, t["src_rows"].ctypes.data, t["src_len"].ctypes.data,
                                               t["rep_rows"].ctypes.data, t["blk_len"].ctypes.data, nb, k, r, L, None)


def _dec_host(lib, t, nb, k, r, L, ctx=None):
    return lib.fecgpu_rlc_decode_rows_len_host(ctx, t["src_rows"].ctypes.data, t["src_len"].ctypes.data,
                                               t["rep_rows"].ctypes.data, t["rep_len"].ctypes.data,
                                               t["blk_len"].ctypes.data, nb, k, r, L, t["seeds"].ctypes.data,
                                               t["sp"].ctypes.data, t["rp"].ctypes.data, t["st"].ctypes.data,
                                               t["rec"].ctypes.data)


@pytest.mark.parametrize("host", [_enc_host, _dec_host])
def test_host_forms_refuse_length_violations(lib, host):
    """src_len <= blk_len <= symbol_size is checked on the host tables before the context is looked at, so
    the refusal is visible without a device: the message names the rule that failed."""
    nb, k, r, L = 3, 4, 2, 1200
    t = _host_tables(nb, k, r, L, blk=1000, src=1000)
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "context" in err(lib)  # lengths fine: only no context
    t = _host_tables(nb, k, r, L, blk=1000, src=1000)
    t["src_len"][nb * k - 1] = 1001
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "src_len" in err(lib)
    t = _host_tables(nb, k, r, L, blk=1000, src=1000)
    t["blk_len"][1] = 1204
    t["src_len"][:] = 0
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "blk_len" in err(lib)
    t = _host_tables(nb, k, r, L, blk=1200, src=1200)  # the limits themselves are accepted
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "context" in err(lib)
    for kw in dict(k=129, r=129, L=1202).items():
        args = dict(k=k, r=r, L=L)
        args[kw[0]] = kw[1]
        assert host(lib, _host_tables(nb, 129, 129, L, 8, 8), nb, args["k"], args["r"], args["L"]) == ERR_INVALID
        assert "context" not in err(lib), kw


def test_decode_host_ignores_the_length_of_a_missing_source(lib):
    nb, k, r, L = 2, 4, 2, 1200
    t = _host_tables(nb, k, r, L, blk=800, src=800)
    t["sp"][:] = 0
    t["sp"][0] = 0b1011
    t["sp"][2] = 0b1111
    t["src_len"][2] = 5000  # block 0, source 2: missing, its length entry is not looked at
    assert _dec_host(lib, t, nb, k, r, L) == ERR_INVALID and "context" in err(lib)
    t["src_len"][4 + 2] = 5000  # block 1, source 2: present
    assert _dec_host(lib, t, nb, k, r, L) == ERR_INVALID and "src_len" in err(lib)


def test_workspace_is_monotone_and_holds_its_parts(lib):
    ws, dws = lib.fecgpu_rlc_rows_len_workspace, lib.fecgpu_rlc_decode_workspace
    for k, r, L in ((1, 1, 4), (16, 4, 1200), (64, 16, 9000), (128, 128, 65532), (8, 0, 1200)):
        prev = 0
        for nb in (0, 1, 2, 3, 64, 65, 4096, 1 << 16):
            n = ws(nb, k, r, L)
            assert n >= prev, (k, r, L, nb)
            assert n >= dws(nb, k, r) + nb * (k + r + min(k, r)) * L, (k, r, L, nb)
            prev = n
    assert ws(0, 16, 4, 1200) == 0
