"""The one-pass ragged-row entry points (fecgpu_rlc_*_rows_fused and their host forms) through the C ABI,
without a GPU: the four symbols, their Python mirrors and the argument checks that come before any launch.
No device call is made: every refused call returns before it touches HIP, and the host forms check their
tables and lengths before they look at the context."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID, ERR_NOMEM = 0, -1, -4

SYMBOLS = ("fecgpu_rlc_encode_rows_fused", "fecgpu_rlc_decode_rows_fused", "fecgpu_rlc_encode_rows_fused_host",
           "fecgpu_rlc_decode_rows_fused_host")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from pquic_amd.engine import load_library
    lib = load_library(LIB, private=True)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    return lib


def test_built_lens_header_is_what_the_generator_writes(tmp_path):
    """The length-aware bodies are not kept in the repository: the build writes csrc/bitslice_lens_gen.h.  The
    header the library was built from is exactly what gen_bitslice.py writes with its defaults, and writing
    it leaves bitslice_gen.h alone (the generator's byte-model check of the length logic runs on the way)."""
    import subprocess
    import sys
    csrc = os.path.join(ROOT, "pquic_amd", "csrc")
    built = os.path.join(csrc, "bitslice_lens_gen.h")
    assert os.path.exists(built), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FEC_GEN")}
    env["FEC_GEN_OUT"] = str(tmp_path / "bitslice_gen.h")
    subprocess.run([sys.executable, os.path.join(csrc, "gen_bitslice.py"), "--lens-only"], env=env, check=True,
                   capture_output=True)
    assert not (tmp_path / "bitslice_gen.h").exists()
    text = (tmp_path / "bitslice_lens_gen.h").read_text()
    assert text == open(built).read()
    for rt in (1, 2, 4, 8, 16):
        for vec in (16, 8, 4):
            assert f"void bs_decl_r{rt}_v{vec}(" in text
    assert "global_load" not in text and "global_store" not in text  # every row access is bounded by a descriptor


def err(lib):
    return lib.fecgpu_last_error().decode()


def test_symbols_are_exported_and_declared(lib):
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name + "(" in text, name


def test_engine_has_the_methods():
    from pquic_amd.engine import Engine, HostPath
    for cls in (Engine, HostPath):
        for m in ("rlc_encode_rows_fused", "rlc_decode_rows_fused"):
            assert inspect.isfunction(getattr(cls, m, None)), (cls.__name__, m)
    # encode takes no workspace
    assert "workspace" not in inspect.signature(Engine.rlc_encode_rows_fused).parameters


# a buffer that stands for every table: never read by a refused call
BUF = np.zeros(1 << 12, np.uint64)
P = BUF.ctypes.data


def _encode(lib, src_rows=P, src_len=P, rep_rows=P, blk_len=P, nb=2, k=4, r=2, L=16):
    return lib.fecgpu_rlc_encode_rows_fused(src_rows, src_len, rep_rows, blk_len, nb, k, r, L, 0, None, None)


def _decode(lib, src_rows=P, src_len=P, rep_rows=P, rep_len=P, blk_len=P, nb=2, k=4, r=2, L=16, seed=P, sp=P, rp=P,
            st=P, rec=P, ws=P, wsb=1 << 15):
    return lib.fecgpu_rlc_decode_rows_fused(src_rows, src_len, rep_rows, rep_len, blk_len, nb, k, r, L, seed, sp, rp,
                                            st, rec, ws, wsb, None)


def test_null_tables_are_refused(lib):
    for kw in ("src_rows", "src_len", "rep_rows", "blk_len"):
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
    assert _encode(lib, src_rows=P + 2) == ERR_INVALID  # the tables are 4-byte aligned like every buffer


def test_empty_batches_are_accepted_without_a_launch(lib):
    assert _encode(lib, nb=0) == OK
    assert _decode(lib, nb=0) == OK
    assert _encode(lib, r=0) == OK  # no repair to write


def test_decode_workspace_is_the_plans(lib):
    need = lib.fecgpu_rlc_decode_workspace(2, 4, 2)
    assert need > 0
    assert _decode(lib, wsb=need - 1) == ERR_NOMEM
    assert lib.fecgpu_rlc_rows_len_workspace(2, 4, 2, 16) > need  # the staged forms' scratch is not asked for


def _host_tables(nb, k, r, L, blk, src):
    return dict(src_rows=np.zeros(nb * k, np.uint64), src_len=np.full(nb * k, src, np.uint32),
                rep_rows=np.zeros(nb * r, np.uint64), rep_len=np.full(nb * r, blk, np.uint32),
                blk_len=np.full(nb, blk, np.uint32), seeds=np.zeros(nb * r, np.uint32),
                sp=np.full(2 * nb, 0xF, np.uint64), rp=np.full(2 * nb, 0x3, np.uint64), st=np.full(nb, 0xEE, np.uint8),
                rec=np.full(2 * nb, 0x55, np.uint64))


def _enc_host(lib, t, nb, k, r, L, ctx=None):
    return lib.fecgpu_rlc_encode_rows_fused_host(ctx, t["src_rows"].ctypes.data, t["src_len"].ctypes.data,
                                                 t["rep_rows"].ctypes.data, t["blk_len"].ctypes.data, nb, k, r, L,
                                                 None)


def _dec_host(lib, t, nb, k, r, L, ctx=None):
    return lib.fecgpu_rlc_decode_rows_fused_host(ctx, t["src_rows"].ctypes.data, t["src_len"].ctypes.data,
                                                 t["rep_rows"].ctypes.data, t["rep_len"].ctypes.data,
                                                 t["blk_len"].ctypes.data, nb, k, r, L, t["seeds"].ctypes.data,
                                                 t["sp"].ctypes.data, t["rp"].ctypes.data, t["st"].ctypes.data,
                                                 t["rec"].ctypes.data)


@pytest.mark.parametrize("host", [_enc_host, _dec_host])
def test_host_forms_refuse_length_violations(lib, host):
    """src_len <= blk_len <= symbol_size is checked on the host tables before the context is looked at, so
    the refusal is visible without a device; nothing is written."""
    nb, k, r, L = 3, 4, 2, 1200
    t = _host_tables(nb, k, r, L, blk=1000, src=1000)
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "context" in err(lib)  # lengths fine: only no context
    t = _host_tables(nb, k, r, L, blk=1000, src=1000)
    t["src_len"][nb * k - 1] = 1001
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "src_len" in err(lib)
    assert (t["st"] == 0xEE).all() and (t["rec"] == 0x55).all()
    t = _host_tables(nb, k, r, L, blk=1000, src=1000)
    t["blk_len"][1] = 1204
    t["src_len"][:] = 0
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "blk_len" in err(lib)
    assert (t["st"] == 0xEE).all() and (t["rec"] == 0x55).all()
    t = _host_tables(nb, k, r, L, blk=1200, src=1200)  # the limits themselves are accepted
    assert host(lib, t, nb, k, r, L) == ERR_INVALID and "context" in err(lib)
    for name, val in dict(k=129, r=129, L=1202).items():
        args = dict(k=k, r=r, L=L)
        args[name] = val
        assert host(lib, _host_tables(nb, 129, 129, L, 8, 8), nb, args["k"], args["r"], args["L"]) == ERR_INVALID
        assert "context" not in err(lib), name


def test_host_forms_refuse_null_tables(lib):
    nb, k, r, L = 2, 4, 2, 64
    for key in ("src_rows", "src_len", "rep_rows", "blk_len"):
        t = _host_tables(nb, k, r, L, 64, 64)
        args = [t[x].ctypes.data if x != key else None for x in ("src_rows", "src_len", "rep_rows", "blk_len")]
        assert lib.fecgpu_rlc_encode_rows_fused_host(None, *args, nb, k, r, L, None) == ERR_INVALID
        assert "NULL row" in err(lib), key
