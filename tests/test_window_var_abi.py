"""Window encode on windows of their own length through the C ABI, without a GPU: the two symbols and their
Python mirrors, the refusals of the host form (each returns before HIP is touched, with a message naming the
rule), the empty call, and fecgpu_rlc_window_classes (pure host code) against a numpy model."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID = 0, -1

SYMBOLS = ("fecgpu_rlc_window_encode_rows_var_host", "fecgpu_rlc_window_classes")


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
    # the device form stays internal: no prototype of the public header carries its name
    assert "fecgpu_rlc_window_encode_rows_var_internal" not in text
    assert not hasattr(lib, "fecgpu_rlc_window_encode_rows_var_internal")


def test_python_mirrors():
    import pquic_amd
    from pquic_amd.engine import HostPath, window_classes
    assert inspect.isfunction(getattr(HostPath, "rlc_window_encode_rows_var", None))
    assert inspect.isfunction(window_classes) and "window_classes" in pquic_amd.__all__


# ------------------------------------------------------------------------------------------ the host form
def _tables(nrows, wrow, wlen, r, row, blk):
    nwin = len(wrow)
    return dict(rows=np.zeros(max(nrows, 1), np.uint64), row_len=np.full(max(nrows, 1), row, np.uint32),
                wrow=np.array(list(wrow) + [0], np.uint32), wlen=np.array(list(wlen) + [1], np.uint8),
                rep_rows=np.zeros(nwin * r + 1, np.uint64), blk_len=np.full(nwin + 1, blk, np.uint32))


def _host(lib, t, nrows, nwin, kmax, r, L, ctx=None):
    return lib.fecgpu_rlc_window_encode_rows_var_host(
        ctx, t["rows"].ctypes.data, t["row_len"].ctypes.data, nrows, t["wrow"].ctypes.data, t["wlen"].ctypes.data,
        t["rep_rows"].ctypes.data, t["blk_len"].ctypes.data, nwin, kmax, r, L)


NROWS, KMAX, R, L = 40, 30, 2, 1200
WROW, WLEN = [0, 1, 8, 10, 3], [30, 7, 1, 30, 12]


def good():
    return _tables(NROWS, WROW, WLEN, R, 1000, 1000)


def test_only_the_context_is_missing(lib):
    """every table is good: the call gets as far as the context, which is looked at last"""
    assert _host(lib, good(), NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "context" in err(lib)
    # the limits themselves: a window that ends on the stream's last row, a length of kmax, a length of 1
    t = good()
    t["wrow"][3] = NROWS - 30
    t["blk_len"][1] = 7  # a row longer than its window is truncated for it, not refused
    assert _host(lib, t, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "context" in err(lib)


def test_refuses_null_tables(lib):
    class Null:  # stands for a NULL table
        class ctypes:
            data = None
    for name in ("rows", "row_len", "wrow", "wlen", "rep_rows", "blk_len"):
        bad = good()
        bad[name] = Null
        assert _host(lib, bad, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID, name
        assert "NULL" in err(lib) and "context" not in err(lib), name


def test_refuses_shapes(lib):
    for kk, rr, LL, word in ((0, R, L, "k out of range"), (129, R, L, "k out of range"), (KMAX, 0, L, "r out of range"),
                             (KMAX, 129, L, "r out of range"), (KMAX, R, 0, "symbol_size"), (KMAX, R, 6, "symbol_size"),
                             (KMAX, R, 1202, "symbol_size"), (KMAX, R, 65536, "symbol_size")):
        assert _host(lib, good(), NROWS, len(WROW), kk, rr, LL) == ERR_INVALID, (kk, rr, LL)
        assert word in err(lib) and "context" not in err(lib), (kk, rr, LL, err(lib))


def test_refuses_window_lengths_and_starts(lib):
    for bad_len in (0, KMAX + 1, 255):
        t = good()
        t["wlen"][2] = bad_len
        assert _host(lib, t, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "wlen" in err(lib), bad_len
    t = good()
    t["wrow"][4] = NROWS - 12 + 1  # 29 + 12 > 40
    assert _host(lib, t, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "wrow" in err(lib)
    t = good()
    t["wrow"][2] = NROWS  # a window of one row, one row past the stream
    assert _host(lib, t, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "wrow" in err(lib)


def test_refuses_lengths_above_symbol_size(lib):
    t = good()
    t["row_len"][NROWS - 1] = L + 1
    assert _host(lib, t, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "row_len" in err(lib)
    t = good()
    t["blk_len"][4] = L + 4
    assert _host(lib, t, NROWS, len(WROW), KMAX, R, L) == ERR_INVALID and "blk_len" in err(lib)


def test_the_empty_call_is_accepted_without_a_launch(lib):
    t = _tables(8, [], [], 2, 16, 16)
    assert _host(lib, t, 8, 0, 4, 2, 16, ctx=1) == OK  # no window: the context is not dereferenced
    assert _host(lib, t, 0, 0, 128, 128, 65532, ctx=1) == OK


# ------------------------------------------------------------------------------------------ the sort
def classes(lib, wlen, kmax, S):
    wlen = np.ascontiguousarray(wlen, np.uint8)
    perm = np.full(len(wlen) + 1, 0xDEADBEEF, np.uint32)
    cls = np.full(4 * kmax + 1, 0xDEADBEEF, np.uint32)
    nc, nch = C.c_uint32(77), C.c_uint64(77)
    rc = lib.fecgpu_rlc_window_classes(wlen.ctypes.data, len(wlen), kmax, S, perm.ctypes.data, cls.ctypes.data,
                                       C.byref(nc), C.byref(nch))
    assert rc == OK, err(lib)
    assert perm[-1] == 0xDEADBEEF and cls[-1] == 0xDEADBEEF, "written past the tables"
    return perm[:-1], cls[:-1].reshape(4, kmax), nc.value, nch.value


def model(wlen, kmax, S):
    """numpy: a stable sort by length, the classes in order of length, each cut into 2 KiB chunks of its own"""
    wlen = np.asarray(wlen, np.int64)
    W = (S + 15) // 16 * 16
    perm = np.argsort(wlen, kind="stable").astype(np.uint32)
    lens = np.unique(wlen)
    cnt = np.array([(wlen == x).sum() for x in lens], np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    chunks = (cnt * W + 2047) // 2048
    cchunk = np.concatenate([[0], np.cumsum(chunks)[:-1]])
    return perm, first, cnt, lens, cchunk, int(chunks.sum())


def check(lib, wlen, kmax, S):
    perm, cls, nc, nch = classes(lib, wlen, kmax, S)
    mperm, first, cnt, lens, cchunk, mch = model(wlen, kmax, S)
    assert nc == len(lens) and nch == mch
    assert np.array_equal(perm, mperm), "the permutation is the stable one"
    assert np.array_equal(cls[0, :nc], first) and np.array_equal(cls[1, :nc], cnt)
    assert np.array_equal(cls[2, :nc], lens) and np.array_equal(cls[3, :nc], cchunk)
    assert not cls[:3, nc:].any() and (cls[3, nc:] == 0xFFFFFFFF).all()
    return cls, nc, nch


def test_classes_match_the_model_on_random_lengths(lib):
    rng = np.random.default_rng(2024)
    for i in range(200):
        kmax = (1, 16, 30, 128)[i % 4]
        nwin = int(rng.integers(1, 501))
        S = int(rng.choice([4, 44, 48, 1200, 1500, 2064, 65532]))
        if i % 3 == 0:  # a walk, as a sender's window grows and shrinks
            wlen = np.clip(np.cumsum(rng.integers(-3, 4, nwin)) + kmax // 2, 1, kmax)
        else:
            wlen = rng.integers(1, kmax + 1, nwin)
        check(lib, wlen, kmax, S)


def test_one_class(lib):
    cls, nc, nch = check(lib, [7] * 100, 30, 1200)
    assert nc == 1 and list(cls[:, 0]) == [0, 100, 7, 0] and nch == (100 * 1200 + 2047) // 2048


def test_every_length_once(lib):
    for kmax in (30, 128):
        wlen = list(range(kmax, 0, -1))
        cls, nc, nch = check(lib, wlen, kmax, 1200)
        assert nc == kmax and nch == kmax and list(cls[3]) == list(range(kmax))
        perm = classes(lib, wlen, kmax, 1200)[0]
        assert list(perm) == list(range(kmax - 1, -1, -1))


def test_a_class_of_whole_chunks_leaves_no_padding(lib):
    """128 windows at width 48 are 6144 B = 3 whole chunks: the next class begins on chunk 3"""
    wlen = [9] * 5 + [4] * 128 + [9] * 6
    cls, nc, nch = check(lib, wlen, 30, 48)
    assert nc == 2 and list(cls[:, 0]) == [0, 128, 4, 0] and list(cls[:, 1]) == [128, 11, 9, 3] and nch == 4
    cls, nc, nch = check(lib, [4] * 129 + [9], 30, 44)  # symbol_size 44: the width is 48; one window more, one chunk more
    assert list(cls[3, :2]) == [0, 4] and nch == 5


def test_classes_refusals(lib):
    wlen = np.array([1, 2, 3], np.uint8)
    perm, cls = np.zeros(3, np.uint32), np.zeros(4 * 128, np.uint32)
    nc, nch = C.c_uint32(0), C.c_uint64(0)

    def call(wl=wlen.ctypes.data, kmax=30, S=1200, p=perm.ctypes.data, c=cls.ctypes.data, a=C.byref(nc), b=C.byref(nch)):
        return lib.fecgpu_rlc_window_classes(wl, 3, kmax, S, p, c, a, b)
    assert call() == OK
    for kw in ("wl", "p", "c", "a", "b"):
        assert call(**{kw: None}) == ERR_INVALID and "NULL" in err(lib), kw
    for kmax in (0, 129):
        assert call(kmax=kmax) == ERR_INVALID and "kmax" in err(lib)
    assert call(kmax=2) == ERR_INVALID and "wlen" in err(lib)
    wlen[1] = 0
    assert call() == ERR_INVALID and "wlen" in err(lib)


def test_python_window_classes_matches_the_model(lib):
    from pquic_amd.engine import FecGpuError, window_classes
    wlen = [3, 1, 3, 30, 1, 3]
    perm, first, cnt, lens, cchunk, nch = window_classes(wlen, 30, 1200)
    m = model(wlen, 30, 1200)
    for got, want in zip((perm, first, cnt, lens, cchunk), m[:5]):
        assert np.array_equal(got, want)
    assert nch == m[5] == 2 + 2 + 1
    with pytest.raises(FecGpuError, match="wlen"):
        window_classes([31], 30, 1200)
