"""The knob ledger: every knob of the engine's table (FEC_KNOBS, pquic_amd/csrc/fec_engine.hip) beside the GPU
tests that run what its non-default values select against the CPU oracle.

The names come from the table itself, so a knob added without an entry here -- that is, without a test that
checks its kernels -- fails the CPU suite, and so does an entry whose test is gone or no longer names the
knob.  No device call is made."""
import ast
import ctypes as C
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so")
ENGINE = os.path.join(ROOT, "pquic_amd", "csrc", "fec_engine.hip")
OK = 0

KK = "tests/test_knob_kernels_gpu.py::"
PARITY = "tests/test_gpu_parity.py::"

# knob: {non-default value: the GPU test that runs it against the oracle}.  A knob that changes timing only
# maps to no value and says why ("timing_only"); the tests that drive it are still named.
LEDGER = {
    "plan": {"values": {1: KK + "test_d_plan_kernels_decode", 2: KK + "test_d_plan_kernels_decode",
                        3: KK + "test_d_plan_kernels_decode", 4: KK + "test_d_plan_kernels_decode",
                        5: KK + "test_d_plan_kernels_decode"}},
    "interleave": {"values": {0: KK + "test_a_encode_tiling_group_order",
                              2: PARITY + "test_group_order_knob_vs_oracle",
                              3: KK + "test_a_encode_tiling_group_order"}},
    "group": {"values": {1: KK + "test_a_encode_group_cap", 2: PARITY + "test_decode_apply_packed",
                         3: KK + "test_a_encode_group_cap"}},
    "enc_tile_rt": {"values": {v: KK + "test_a_encode_tiling" for v in (1, 2, 4, 8, 16)}},
    "enc_tile_waves": {"values": {v: KK + "test_a_encode_tiling" for v in (1, 2, 3, 4)}},
    "enc_block_waves": {"values": {2: KK + "test_b_multi_wave_encode_lds",
                                   4: KK + "test_b_multi_wave_encode_lds"}},
    "zc_read": {"values": {0: KK + "test_e_zc_read_0_stages_page_locked_buffers"}},
    "ring": {"values": {0: PARITY + "test_ring_datapath_vs_oracle"}},
    "window_sc": {"values": {0: KK + "test_e_window_encode_kernels", 2: KK + "test_e_window_encode_kernels"}},
    "min_groups": {"values": {0: KK + "test_b_multi_wave_encode_lds"}},
    "chunk_waves": {"values": {0: KK + "test_c_chunk_waves_encode_and_decode"}},
    "small_lds": {"values": {0: PARITY + "test_small_batch_encode_lds_vs_oracle"}},
    "block_svc": {"values": {},
                  "timing_only": "0 refuses every service request, so the caller takes the launch forms tested elsewhere",
                  "tests": ["tests/test_hooks_in_place_gpu.py::test_knob_block_svc_0_takes_the_launch_forms"]},
    "ws_lds": {"values": {0: PARITY + "test_decode_ws_lds_vs_oracle"}},
    "dec_waves": {"values": {v: KK + "test_d_dec_waves_decode" for v in (1, 3, 8)}},
    "yield_slice_kb": {"values": {0: "tests/test_host_rows_gpu.py::test_sliced_equals_unsliced",
                                  1: KK + "test_e_pacer_slices"}},
    "yield_depth": {"values": {1: KK + "test_e_pacer_slices", 2: KK + "test_e_pacer_slices"}},
    "yield_gate_us": {"values": {200: KK + "test_e_pacer_slices"}},
    "yield_streams": {"values": {1: KK + "test_e_pacer_slices", 4: KK + "test_e_pacer_slices"}},
    "yield_always": {"values": {},
                     "timing_only": "slices whether or not a hook ran lately; what a slice computes is yield_slice_kb's",
                     "tests": [KK + "test_e_pacer_slices", "tests/test_host_rows_gpu.py::test_sliced_equals_unsliced"]},
    "yield_window_ms": {"values": {},
                        "timing_only": "how long after a hook request bulk calls keep slicing",
                        "tests": ["tests/test_block_svc_gpu.py::test_bulk_slices_yield_to_hooks_and_keep_the_bytes"]},
    "span_compact": {"values": {0: "tests/test_batch_span_gpu.py::test_knob_parity"}},
}

SYMBOLS = {"PLAN_AUTO": 0}  # defaults the table spells by name


def knob_table(path=ENGINE):
    """[(name, default)] of the engine's own table, in its order."""
    text = open(path).read()
    m = re.search(r"#define FEC_KNOBS\(X\)(.*?)\n\n", text, re.S)
    assert m, "no FEC_KNOBS table in fec_engine.hip"
    body = m.group(1)
    names = re.findall(r'X\(\s*[A-Z0-9_]+\s*,\s*"([a-z0-9_]+)"', body)
    rows = re.findall(r'X\(\s*[A-Z0-9_]+\s*,\s*"([a-z0-9_]+)"\s*,\s*([A-Za-z0-9_]+)\s*,', body)
    assert names and [n for n, _ in rows] == names, "a row of FEC_KNOBS does not parse"
    return [(n, SYMBOLS[d] if d in SYMBOLS else int(d)) for n, d in rows]


def knob_defaults():
    return dict(knob_table())


def ledger_problems(ledger, table):
    """What is wrong with a ledger against a table's names (no library needed): a list of sentences."""
    out = []
    names = [n for n, _ in table]
    for n in names:
        if n not in ledger:
            out.append(f"knob {n} of the table has no ledger entry")
    for n in ledger:
        if n not in names:
            out.append(f"ledger entry {n} names no knob of the table")
    for n, e in ledger.items():
        if not e["values"] and not (e.get("timing_only") and e.get("tests")):
            out.append(f"{n}: no value listed, and no reason with the tests that drive it")
    return out


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = C.CDLL(LIB)
    L.fecgpu_set_knob.argtypes = [C.c_char_p, C.c_int]
    L.fecgpu_get_knob.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    return L


def get(lib, name):
    v = C.c_int(-12345)
    assert lib.fecgpu_get_knob(name.encode(), C.byref(v)) == OK, name
    return v.value


def test_the_ledger_holds_exactly_the_tables_knobs():
    table = knob_table()
    assert len(table) == len(set(n for n, _ in table)) >= 22
    assert not ledger_problems(LEDGER, table)


def test_the_parsed_defaults_are_the_librarys(lib):
    for name, default in knob_table():
        assert get(lib, name) == default, name


@pytest.mark.parametrize("name", sorted(LEDGER))
def test_listed_values_are_accepted_and_not_the_default(lib, name):
    default = knob_defaults()[name]
    assert get(lib, name) == default
    try:
        for v in LEDGER[name]["values"]:
            assert v != default, (name, v)
            assert lib.fecgpu_set_knob(name.encode(), v) == OK, (name, v)
            assert get(lib, name) == v
    finally:
        assert lib.fecgpu_set_knob(name.encode(), default) == OK
    assert get(lib, name) == default


_parsed = {}


def find_test(test_id):
    """The ast of the test a ledger entry names, or None."""
    path, _, func = test_id.partition("::")
    if path not in _parsed:
        full = os.path.join(ROOT, path)
        _parsed[path] = ast.parse(open(full).read()) if os.path.exists(full) else None
    tree = _parsed[path]
    if tree is None:
        return None
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == func:
            return node
    return None


def names_knob(node, name):
    """The knob's name stands in the test's own body as a str or bytes literal."""
    return any(isinstance(c, ast.Constant) and c.value in (name, name.encode()) for c in ast.walk(node))


@pytest.mark.parametrize("name", sorted(LEDGER))
def test_named_tests_exist_and_name_the_knob(name):
    entry = LEDGER[name]
    ids = sorted(set(entry["values"].values()) | set(entry.get("tests", ())))
    assert ids, name
    for test_id in ids:
        node = find_test(test_id)
        assert node is not None, f"{name}: {test_id} does not exist"
        assert "pytest.mark.gpu" in open(os.path.join(ROOT, test_id.partition("::")[0])).read(), test_id
        assert names_knob(node, name), f"{name}: {test_id} does not name the knob"


def test_the_check_notices_a_missing_entry_and_a_renamed_knob():
    """The ledger check itself: one entry fewer, or a table whose knob has another name, is reported."""
    table = knob_table()
    fewer = {n: e for n, e in LEDGER.items() if n != "dec_waves"}
    assert ledger_problems(fewer, table) == ["knob dec_waves of the table has no ledger entry"]
    renamed = [("dec_wave_cap" if n == "dec_waves" else n, d) for n, d in table]
    assert len(ledger_problems(LEDGER, renamed)) == 2
