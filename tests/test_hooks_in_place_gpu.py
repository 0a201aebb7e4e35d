"""The protocol operations with pquic_fec_set_hooks_in_place(1): symbols that lie in a registered (page-locked)
plugin arena are handed to the engine by address, the others go through a staging row, and the block is
served by the resident worker's row requests or, where it refuses, by the launch forms on the same tables.
Driven through the picoquic stand-in (tests/host/mini_host.c) against the reference's fixtures: every case
must give exactly what test_protoops_gpu.py asserts for it with the mode off, whatever mix of rows it runs on.

The stand-in's arena holds symbols up to 2092 bytes (one 2112-byte slot each, picoquic/memory.c); a longer
symbol comes from the heap in every mode, so `rows staged == 0` is asserted over the cases whose symbols
fit a slot and the 9000-byte cases are checked for their results alone."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from golden_io import load, sha, window_inputs
from oracle_py import DEC_RECOVERED, Oracle
from test_protoops_gpu import Host, _decode_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SLOT_DATA = 2092
ERROR_MEMORY = 0x405


@pytest.fixture(scope="module")
def fec():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from pquic_amd import load_library
    L = load_library()
    L.pquic_fec_hook_rows_stats.argtypes = [C.c_void_p]
    L.pquic_fec_hook_rows_stats.restype = None
    L.pquic_fec_singular_blocks.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def host(fec):
    h = Host()
    L = h.lib
    L.mh_arena_enable.argtypes = [C.c_size_t]
    L.mh_arena_live.argtypes = [C.c_int]
    L.mh_arena_live.restype = C.c_long
    L.mh_arena_strict.argtypes = [C.c_int]
    L.mh_fail_next_generate.argtypes = [C.c_long]
    L.mh_fail_alloc_after.argtypes = [C.c_long]
    h.live0 = L.mh_live_allocations()
    h.batcher_open = False
    yield h
    # the process is shared with the other suites: mode off, no batcher, nothing armed
    fec.pquic_fec_set_hooks_in_place(0)
    fec.pquic_fec_set_recover_mode(0)
    fec.fecgpu_set_knob(b"block_svc", 1)
    L.mh_fail_alloc_after(-1)
    L.mh_arena_strict(0)
    if h.batcher_open:
        L.mh_batch_close()


@contextlib.contextmanager
def arena(host, nbytes, strict):
    """A fresh default arena, page-locked through a batcher's registry (the engine's registry is all the
    hooks look at); afterwards the batcher is closed, which takes the arena out of the registry again."""
    L = host.lib
    assert L.mh_arena_enable(nbytes) == 0
    assert L.mh_batch_open(0, 1, 1000, 9000, 2, 0) == 0
    host.batcher_open = True
    assert L.mh_batch_register_arena() == 0
    L.mh_arena_strict(int(strict))
    try:
        yield
        assert L.mh_arena_live(-1) == 0
    finally:
        L.mh_arena_strict(0)
        L.mh_batch_close()
        host.batcher_open = False


@contextlib.contextmanager
def in_place(fec):
    assert fec.pquic_fec_set_hooks_in_place(1) == 0
    try:
        yield
    finally:
        assert fec.pquic_fec_set_hooks_in_place(0) == 0


def stats(fec):
    out = np.zeros(4, np.uint64)
    fec.pquic_fec_hook_rows_stats(out.ctypes.data)
    return [int(x) for x in out]  # rows in place, rows staged, calls served by the worker, calls launched


def delta(fec, s0):
    return [a - b for a, b in zip(stats(fec), s0)]


# ---- the cases of test_protoops_gpu.py, one at a time, with what it asserts for each ----
def check_encode_varlen(host, case):
    srcs = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in case["src_hex"]]
    ret, reps, fps, sch = host.generate(case["scheme"] == "xor", case["fbn"], srcs, case["r"])
    assert ret == case["ret"]
    assert [x.tobytes().hex() for x in reps] == case["rep_hex"]
    assert fps == case["repair_fpid_raw"]
    assert (sch[0] == sch[1] != 0) if case["scheme"] == "rlc" else (sch[0] == sch[1] == 0)


def check_encode_fixed(host, case):
    from golden_io import encode_inputs
    src = encode_inputs(case)
    for b in range(case["nblocks"]):
        fbn = (case["fbn_base"] + b) & 0xFFFFFF
        ret, reps, fps, _ = host.generate(case["scheme"] == "xor", fbn, list(src[b]), case["r"])
        assert ret == 0
        assert sha(np.stack(reps).tobytes()) == case["block_sha256"][b], case["name"]
        assert fps == case["repair_fpid_raw"][b]


def check_decode(host, case):
    (ret, rec, cur), srcs = _decode_case(host, case)
    if case["crashed"]:  # the reference segfaults on this pattern; nothing is recovered
        assert ret == 0 and rec == {}, case["tag"]
        return
    assert ret == case["ret"], case["tag"]
    assert {str(j): sha(v.tobytes()) for j, v in sorted(rec.items())} == case["recovered"], case["tag"]
    assert {str(j): len(v) for j, v in rec.items()} == case["recovered_len"], case["tag"]
    present = sum(s is not None for s in srcs)
    assert cur == (present + len(rec) if case["scheme"] == "rlc" else present), case["tag"]


def check_window(host, oracle, case):
    srcs_full, reps_full, fpids = window_inputs(case, oracle)
    k, r = case["k"], case["r"]
    srcs = [None if j in case["src_missing"] else srcs_full[j] for j in range(k)]
    reps = [reps_full[i] if i in case["rep_present"] else None for i in range(r)]
    ret, rec, cur = host.recover(case["scheme"] == "xor", case["fbn"], srcs, reps, fpids)
    if case["crashed"]:
        assert ret == 0 and rec == {}, case["tag"]
        return
    assert ret == case["ret"], case["tag"]
    assert {str(j): sha(v.tobytes()) for j, v in sorted(rec.items())} == case["recovered"], case["tag"]
    assert {str(j): len(v) for j, v in rec.items()} == case["recovered_len"], case["tag"]
    assert {str(j): f for j, f in host.last_fpids.items()} == case["recovered_fpid"], case["tag"]
    present = sum(s is not None for s in srcs)
    assert cur == (present + len(rec) if case["scheme"] == "rlc" else present), case["tag"]


def golden_cases(fixed):
    """(check, case, fits a slot) for: every varlen encode case, every fixed encode case with k, r <= 100 (with
    `fixed`), the variable-length decode cases, a 60-case slice of the decode cases (XOR and RLC), the five
    reference-crash cases and 20 window-recover cases (XOR and RLC)."""
    e, d, w = load("encode_cases.json"), load("decode_cases.json"), load("window_cases.json")
    o = Oracle()
    out = [(check_encode_varlen, c, max(len(h) // 2 for h in c["src_hex"]) <= SLOT_DATA) for c in e["varlen"]]
    if fixed:
        out += [(check_encode_fixed, c, c["L"] <= SLOT_DATA) for c in e["cases"] if c["k"] <= 100 and c["r"] <= 100]
    out += [(check_decode, c, c["L"] <= SLOT_DATA) for c in d["varlen_cases"]]
    usable = [c for c in d["cases"] if not c["crashed"] and c["k"] <= 100]
    piece = usable[::6][:60]
    assert len(piece) == 60 and {c["scheme"] for c in piece} == {"rlc", "xor"}
    out += [(check_decode, c, c["L"] <= SLOT_DATA) for c in piece]
    crashed = [c for c in d["cases"] if c["crashed"]]
    assert len(crashed) == 5
    out += [(check_decode, c, c["L"] <= SLOT_DATA) for c in crashed]
    win = w["cases"][::8][:20]
    assert len(win) == 20 and {c["scheme"] for c in win} == {"rlc", "xor"}
    out += [(lambda h, c: check_window(h, o, c), c, c["L"] <= SLOT_DATA) for c in win]
    return out


def run_golden(host, fec, fixed=False):
    """Runs the cases; returns the counters' movement over the cases that fit a slot and over the others."""
    small, large = [0] * 4, [0] * 4
    for check, case, fits in golden_cases(fixed):
        s0 = stats(fec)
        check(host, case)
        acc = small if fits else large
        for i, x in enumerate(delta(fec, s0)):
            acc[i] += x
    return small, large


def test_mode_off_moves_no_counter(host, fec):
    assert fec.pquic_fec_get_hooks_in_place() == 0
    small, large = run_golden(host, fec)
    assert small == [0] * 4 and large == [0] * 4


def test_registered_strict_arena_every_row_in_place(host, fec):
    with arena(host, 4 << 20, strict=True), in_place(fec):
        small, large = run_golden(host, fec, fixed=True)
    in_rows, staged_rows, served, launched = small
    assert staged_rows == 0 and in_rows > 0 and served > 0
    assert large[1] > 0  # the 9000-byte symbols come from the heap: staged, with the same results
    assert host.lib.mh_live_allocations() == host.live0


def test_no_arena_every_row_staged_and_xor_on_the_worker(host, fec):
    with in_place(fec):
        small, large = run_golden(host, fec)
        assert small[0] == 0 and large[0] == 0 and small[1] > 0
        # XOR has no launch-free path without the mode; with it the worker serves it, arena or not
        e = load("encode_cases.json")
        s0 = stats(fec)
        nx = 0
        for c in e["varlen"]:
            if c["scheme"] == "xor" and c["ret"] == 0:
                check_encode_varlen(host, c)
                nx += 1
        d = delta(fec, s0)
        assert nx > 0 and d[2] > 0 and d[2] + d[3] == nx  # (a request withdrawn at its deadline is launched)
    assert host.lib.mh_live_allocations() == host.live0


def test_small_arena_mixes_rows_in_place_and_staged(host, fec):
    # 9 slots: a block's first symbols take them, the later ones fall to the heap (not strict)
    with arena(host, 9 * 2112, strict=False), in_place(fec):
        small, _ = run_golden(host, fec)
    assert small[0] > 0 and small[1] > 0 and small[2] > 0
    assert host.lib.mh_live_allocations() == host.live0


def test_knob_block_svc_0_takes_the_launch_forms(host, fec):
    assert fec.fecgpu_set_knob(b"block_svc", 0) == 0
    try:
        with arena(host, 4 << 20, strict=True), in_place(fec):
            small, large = run_golden(host, fec)
    finally:
        assert fec.fecgpu_set_knob(b"block_svc", 1) == 0
    assert small[2] == 0 and large[2] == 0 and small[3] > 0 and small[1] == 0 and small[0] > 0
    assert host.lib.mh_live_allocations() == host.live0


def test_full_rank_mode_in_place(host, fec):
    from test_full_rank_hooks_gpu import _check_recovered, _hook_blocks
    blocks = _hook_blocks()
    given_up = next(b for b in blocks if b["full"] and b["ref_st"] == 2)
    singular = next(b for b in blocks if not b["full"])
    with arena(host, 4 << 20, strict=True), in_place(fec):
        s0 = stats(fec)
        # reference mode: both are given up, nothing inserted
        for blk in (given_up, singular):
            ret, rec, cur = host.recover(False, blk["fbn"], blk["srcs"], blk["reps"], blk["fpids"])
            assert ret == 0 and rec == {} and cur == sum(s is not None for s in blk["srcs"])
        assert fec.pquic_fec_set_recover_mode(1) == 0
        try:
            sing0 = fec.pquic_fec_singular_blocks()
            ret, rec, cur = host.recover(False, given_up["fbn"], given_up["srcs"], given_up["reps"], given_up["fpids"])
            _check_recovered(host, given_up, ret, rec, cur)
            assert fec.pquic_fec_singular_blocks() == sing0
            ret, rec, cur = host.recover(False, singular["fbn"], singular["srcs"], singular["reps"], singular["fpids"])
            assert ret == 0 and rec == {} and cur == sum(s is not None for s in singular["srcs"])
            assert fec.pquic_fec_singular_blocks() == sing0 + 1
        finally:
            assert fec.pquic_fec_set_recover_mode(0) == 0
        d = delta(fec, s0)
        assert d[1] == 0 and d[2] > 0 and d[2] + d[3] == 4
    assert host.lib.mh_live_allocations() == host.live0


def _generate_with_failure(host, xor, fbn, srcs, r, n):
    live = host.lib.mh_live_allocations()
    host.lib.mh_fail_next_generate(n)
    ret, reps, fps, _ = host.generate(xor, fbn, srcs, r)
    return ret, [x.tobytes() for x in reps], fps, host.lib.mh_live_allocations() - live


@pytest.mark.parametrize("xor,k,r", [(False, 16, 4), (True, 4, 1)])
def test_generate_allocation_failures_match_the_staged_hook(host, fec, xor, k, r):
    """The n-th allocation of the operation fails, for every n up to 2r (2r: none does).  Both modes allocate
    the repairs in the same order -- symbol, data, symbol, data -- so the return value, the attached repairs
    and the live allocations agree exactly."""
    rng = np.random.default_rng(5 + k)
    srcs = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(1, 1201, k)]
    srcs[1] = rng.integers(0, 256, 1200, dtype=np.uint8)
    want = [_generate_with_failure(host, xor, 4242, srcs, r, n) for n in range(2 * r + 1)]
    assert [w[0] for w in want] == [ERROR_MEMORY] * (2 * r) + [0]
    assert all(w[3] == 0 for w in want)
    with arena(host, 4 << 20, strict=True), in_place(fec):
        s0 = stats(fec)
        for n in range(2 * r + 1):
            assert _generate_with_failure(host, xor, 4242, srcs, r, n) == want[n], n
        assert delta(fec, s0)[1] == 0
    assert host.lib.mh_live_allocations() == host.live0


@pytest.mark.parametrize("xor", [False, True])
def test_recover_allocation_failures(host, fec, xor):
    """One of the operation's first allocations fails.  The recovered symbols are allocated before the engine
    call and a failed one is allocated again afterwards, as the batcher does it: the reference's rule for the
    value (RLC 0 whatever it could insert, rlc_fec_scheme_gf256.c:222-226,250; XOR 0 after an insertion, else
    PICOQUIC_ERROR_MEMORY), the oracle's bytes in every inserted symbol, nothing leaked."""
    o = Oracle()
    rng = np.random.default_rng(77 + xor)
    k, r, fbn = (4, 1, 91) if xor else (16, 4, 92)
    full = [rng.integers(1, 256, int(n), dtype=np.uint8) for n in rng.integers(1, 1201, k)]
    full[0] = rng.integers(1, 256, 1200, dtype=np.uint8)
    miss = [2] if xor else [2, 5, 11]
    reps = [o.xor_encode_block(full)[1]] if xor else o.rlc_encode_block(fbn, full, r)[1]
    srcs = [None if j in miss else full[j] for j in range(k)]
    st, want = (o.xor_decode_block(srcs, reps) if xor else o.rlc_decode_block(fbn, srcs, reps))
    assert st == DEC_RECOVERED and sorted(want) == miss
    built = (0 if xor else 1) + 2 * (k - len(miss)) + 2 * r  # allocations before the operation's own
    with arena(host, 4 << 20, strict=True), in_place(fec):
        for n in range(7):
            live = host.lib.mh_live_allocations()
            host.lib.mh_fail_alloc_after(built + n)
            try:
                ret, rec, cur = host.recover(xor, fbn, srcs, reps, [(fbn << 8) | i for i in range(r)])
            finally:
                host.lib.mh_fail_alloc_after(-1)
            assert ret == (0 if (rec or not xor) else ERROR_MEMORY), n
            assert set(rec) <= set(miss), n
            for j, row in rec.items():
                assert np.array_equal(row, want[j]), (n, j)
            assert cur == (k - len(miss) if xor else k - len(miss) + len(rec)), n
            assert host.lib.mh_live_allocations() == live, n
    assert host.lib.mh_live_allocations() == host.live0


def test_everything_returned(host, fec):
    assert fec.pquic_fec_get_hooks_in_place() == 0
    assert host.lib.mh_live_allocations() == host.live0
    assert host.lib.mh_arena_live(-1) == 0
