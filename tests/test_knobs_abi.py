"""The engine's knob table through the C ABI, without a GPU: every knob's default, the values it
accepts and refuses, the names that are gone, and the header's list of them.  No device call is made."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
OK, ERR_INVALID = 0, -1

# name: (default, an accepted non-default value, a rejected value)
KNOBS = {
    "plan": (0, 5, 6),
    "interleave": (1, 3, 4),
    "group": (0, 7, -1),
    "enc_tile_rt": (0, 8, 3),
    "enc_tile_waves": (0, 4, 5),
    "enc_block_waves": (1, 4, 3),
    "zc_read": (1, 0, 2),
    "ring": (2, 0, 1),
    "window_sc": (1, 2, 3),
    "min_groups": (1024, 0, -1),
    "chunk_waves": (1, 0, 2),
    "small_lds": (1, 0, 2),
    "block_svc": (1, 0, -1),
    "ws_lds": (1, 0, 2),
    "dec_waves": (0, 8, 9),
    "yield_slice_kb": (2304, 0, (1 << 20) + 1),
    "yield_depth": (16, 1, 17),
    "yield_gate_us": (0, 10000, 10001),
    "yield_streams": (2, 4, 5),
    "yield_always": (0, 1, 2),
    "yield_window_ms": (100, 600000, 600001),
}
REMOVED = ("svc_reserve_cus", "zc_cus", "host_alloc")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = C.CDLL(LIB)
    L.fecgpu_set_knob.argtypes = [C.c_char_p, C.c_int]
    L.fecgpu_get_knob.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    return L


def get(lib, name):
    v = C.c_int(-12345)
    rc = lib.fecgpu_get_knob(name.encode() if name is not None else None, C.byref(v))
    return rc, v.value


@pytest.mark.parametrize("name", sorted(KNOBS))
def test_default_accept_reject_restore(lib, name):
    default, good, bad = KNOBS[name]
    assert good != default
    assert get(lib, name) == (OK, default)
    try:
        assert lib.fecgpu_set_knob(name.encode(), good) == OK
        assert get(lib, name) == (OK, good)
        assert lib.fecgpu_set_knob(name.encode(), bad) == ERR_INVALID
        assert get(lib, name) == (OK, good)  # a refused value changes nothing
    finally:
        assert lib.fecgpu_set_knob(name.encode(), default) == OK
    assert get(lib, name) == (OK, default)


@pytest.mark.parametrize("name", REMOVED + ("no_such_knob", "", None))
def test_unknown_names_are_refused(lib, name):
    raw = name.encode() if name is not None else None
    assert lib.fecgpu_set_knob(raw, 0) == ERR_INVALID
    rc, v = get(lib, name)
    assert rc == ERR_INVALID and v == -12345
    assert lib.fecgpu_get_knob(b"plan", None) == ERR_INVALID  # NULL value pointer


def test_ring_is_rt16_only(lib):
    for v in (4, 8):
        assert lib.fecgpu_set_knob(b"ring", v) == ERR_INVALID
    assert get(lib, "ring") == (OK, 2)


def test_set_valued_knobs(lib):
    """The knobs whose accepted values are a set, not a range: every member and the gaps between."""
    for name, members, lo, hi in (("enc_tile_rt", {0, 1, 2, 4, 8, 16}, -1, 17), ("enc_block_waves", {1, 2, 4}, 0, 5),
                                  ("ring", {0, 2}, -1, 9)):
        try:
            for v in range(lo, hi + 1):
                assert lib.fecgpu_set_knob(name.encode(), v) == (OK if v in members else ERR_INVALID), (name, v)
        finally:
            assert lib.fecgpu_set_knob(name.encode(), KNOBS[name][0]) == OK


def test_header_lists_exactly_the_knobs(lib):
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+fecgpu_set_knob\s*\(", text, re.S)
    assert m, "no comment above fecgpu_set_knob"
    listed = set(re.findall(r'"([a-z0-9_]+)"', m.group(1)))
    assert listed == set(KNOBS)
    for name in listed:
        assert get(lib, name)[0] == OK, name
