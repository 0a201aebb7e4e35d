"""The resident block service's row requests (fecgpu_block_svc_*_rows, include/fecgpu.h): one block per
call with every row given by its address and its own length.  Byte work: every comparison is exact.

Every row sits in its own slice of one page-locked buffer, at an offset that is 0, 4, 8 or 12 mod 16 by
turns; the bytes between a row's length and the next row hold 0xA5.  After each call the whole buffer is
compared with the expected image, so an output row holds exactly its blk_len bytes, every input row is
untouched and no guard byte changed -- and since the guards are not zero, a load that let the bytes after a
row's length into the arithmetic shows in the output.  Every address handed to the worker is a live one,
or 0 where the interface says the row is never dereferenced."""
import ctypes as C

import numpy as np
import pytest

from decode_full_cases import RECOVERED, REF_UB, SINGULAR, TUPLES, case
from oracle_py import DEC_NOTHING, DEC_RECOVERED, DEC_REF_UB, Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
GUARD = 0xA5
OK, ERR_INVALID = 0, -1
SERVE_DEADLINE_US = 1_000_000  # as test_block_svc_gpu.py: never withdrawn because a fresh box was slow
SHAPES = [(1, 1, 1), (5, 3, 19), (16, 4, 1200), (16, 4, 1198), (32, 8, 1201), (20, 16, 37), (64, 16, 100), (100, 100, 8)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from pquic_amd import load_library
    return load_library()


@pytest.fixture(scope="module")
def eng(lib):
    from pquic_amd import Engine
    return Engine(0)


@pytest.fixture(scope="module")
def svc(lib):
    v = lib.fecgpu_block_svc_create(0)
    assert v
    assert lib.fecgpu_block_svc_set_deadline(v, SERVE_DEADLINE_US) == 0
    yield v
    lib.fecgpu_block_svc_destroy(v)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def to_dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(a):
    return a.ctypes.data


def mask(bits):
    m = np.zeros(2, np.uint64)
    for j in bits:
        m[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return m


def bits(m, n):
    return [j for j in range(n) if (int(m[j >> 6]) >> (j & 63)) & 1]


class Pool:
    """Rows in one byte pool: row q starts at 0, 4, 8 or 12 mod 16 (by turns) and at least 24 guard bytes
    follow its room."""

    def __init__(self):
        self.end, self.n = 64, 0

    def add(self, room):
        o = ((self.end + 15) & ~15) + 4 * (self.n % 4)
        self.n += 1
        self.end = o + room + 24
        return o

    def image(self):
        return np.full(self.end + 64, GUARD, np.uint8)


class Pinned:
    """The pool's image in page-locked memory, and the device address of its first byte."""

    def __init__(self, lib, image):
        self.t = torch.from_numpy(image.copy()).pin_memory()
        self.h = self.t.numpy()
        d = C.c_uint64(0)
        assert lib.fecgpu_host_device_address(self.t.data_ptr(), self.h.size, C.byref(d)) == 0
        self.base = d.value
        assert self.base % 16 == 0


def addrs(base, offs):
    return np.array([0 if o is None else base + o for o in offs], np.uint64)


def ragged(rng, k, B):
    """Source lengths that include 0, 1, B - 1 and B (as far as k allows), the rest random."""
    lens = [int(x) for x in rng.integers(0, B + 1, k)]
    for j, n in zip(rng.permutation(k), (B, 0, 1, B - 1)):
        lens[j] = max(n, 0)
    return lens


# ------------------------------------------------------------------------------------------ RLC encode
class EncCase:
    def __init__(self, oracle, k, r, B, seed, xor=False):
        rng = np.random.default_rng(seed)
        self.k, self.r, self.B, self.fbn = k, r, B, int(rng.integers(0, 1 << 24))
        self.lens = ragged(rng, k, B)
        p = Pool()
        self.src_off = [p.add(n) if n else None for n in self.lens]  # a row of 0 bytes: address 0
        self.rep_off = [p.add(B) for _ in range(r)]
        self.image = p.image()
        padded = []
        for n, o in zip(self.lens, self.src_off):
            row = np.zeros(B, np.uint8)
            row[:n] = rng.integers(0, 256, n, dtype=np.uint8)
            if n:
                self.image[o:o + n] = row[:n]
            padded.append(row)
        ret, reps = oracle.xor_encode_block(padded) if xor else oracle.rlc_encode_block(self.fbn, padded, r)
        assert ret == 0
        self.want = self.image.copy()
        for o, rep in zip(self.rep_off, [reps] if xor else reps):
            assert len(rep) == B
            self.want[o:o + B] = rep
        self.src_len = np.array(self.lens, np.uint32)


def svc_encode(lib, svc, c, base):
    rows, reps = addrs(base, c.src_off), addrs(base, c.rep_off)
    return lib.fecgpu_block_svc_rlc_encode_rows(svc, ptr(rows), ptr(c.src_len), ptr(reps), c.B, c.k, c.r, c.fbn)


@pytest.mark.parametrize("k,r,B", SHAPES)
def test_rlc_encode_matches_the_oracle(lib, svc, eng, oracle, k, r, B):
    c = EncCase(oracle, k, r, B, 100 * k + r + B)
    pin = Pinned(lib, c.image)
    assert svc_encode(lib, svc, c, pin.base) == OK, lib.fecgpu_last_error()
    assert np.array_equal(pin.h, c.want), (k, r, B, np.flatnonzero(pin.h != c.want)[:8])
    if (k, r, B) == (16, 4, 1198):  # and byte for byte what the launch form writes on the same tables
        pool = to_dev(c.image)
        L = (B + 3) & ~3
        eng.rlc_encode_rows_fused(to_dev(addrs(pool.data_ptr(), c.src_off)), to_dev(c.src_len),
                                  to_dev(addrs(pool.data_ptr(), c.rep_off)), to_dev(np.array([B], np.uint32)), 1, k, r,
                                  L, fbn=to_dev(np.array([c.fbn], np.uint32)))
        torch.cuda.synchronize()
        assert np.array_equal(pool.cpu().numpy(), pin.h)


# ------------------------------------------------------------------------------------------ RLC decode
class DecCase:
    """A block of ragged sources with `miss` missing and the repairs `present` received.  One received source
    is longer than the block (when one is received): it is read for blk_len bytes."""

    def __init__(self, oracle, k, r, B, miss, present, seed, fbn=None, src=None):
        rng = np.random.default_rng(seed)
        self.k, self.r, self.B = k, r, B
        self.fbn = int(rng.integers(0, 1 << 24)) if fbn is None else fbn
        self.miss, self.present = sorted(int(j) for j in miss), sorted(int(i) for i in present)
        lens = ragged(rng, k, B)
        padded = []
        for j, n in enumerate(lens):
            row = np.zeros(B, np.uint8)
            row[:n] = rng.integers(0, 256, n, dtype=np.uint8) if src is None else src[j][:n]
            padded.append(row)
        ret, reps = oracle.rlc_encode_block(self.fbn, padded, r)
        assert ret == 0 and all(len(x) == B for x in reps)
        self.seeds = np.array([(self.fbn << 8) | i for i in range(r)], np.uint32)
        got = [j for j in range(k) if j not in self.miss]
        self.long = got[len(got) // 2] if got else None
        p = Pool()
        self.src_off, self.rep_off = [], []
        self.src_len = np.zeros(k, np.uint32)
        given = []
        for j in range(k):
            if j in self.miss:
                self.src_off.append(p.add(B))  # where the recovered bytes go
                given.append(None)
                self.src_len[j] = 0xDEAD  # an absent row's length is not looked at
                continue
            data = padded[j][:lens[j]]
            if j == self.long:  # 8 bytes more than the block: truncated (rlc_fec_scheme_gf256.c:205)
                data = np.concatenate([padded[j], rng.integers(1, 256, 8, dtype=np.uint8)])
            self.src_len[j] = len(data)
            self.src_off.append(p.add(len(data)) if len(data) else None)
            given.append(data)
        for i in range(r):
            self.rep_off.append(p.add(B) if i in self.present else None)  # an absent repair: address 0
        self.rep_len = np.array([B if i in self.present else 0xBEEF for i in range(r)], np.uint32)
        self.image = p.image()
        for o, d in zip(self.src_off, given):
            if d is not None and len(d):
                self.image[o:o + len(d)] = d
        for i in self.present:
            self.image[self.rep_off[i]:self.rep_off[i] + B] = reps[i]
        self.sp, self.rp = mask(got), mask(self.present)
        self.st, self.out = oracle.rlc_decode_block(self.fbn, given, [reps[i] if i in self.present else None
                                                                    for i in range(r)],
                                                    rep_seeds=[int(x) for x in self.seeds])
        self.padded = padded

    def check(self, pin_h, st, rec, want_st, want_out, tag):
        """status, mask and the whole buffer: recovered rows hold their B bytes; a missing source of a RECOVERED
        block whose bit stays clear may have received B unspecified bytes; nothing else changed."""
        assert st == want_st, tag
        assert bits(rec, self.k) == sorted(want_out), tag
        want = self.image.copy()
        for j, row in want_out.items():
            assert len(row) == self.B
            want[self.src_off[j]:self.src_off[j] + self.B] = row
        got = pin_h.copy()
        if want_st == DEC_RECOVERED:
            for j in self.miss:
                if j not in want_out:
                    got[self.src_off[j]:self.src_off[j] + self.B] = GUARD
        assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:8])


def svc_decode(lib, svc, c, base, full=0):
    rows, reps = addrs(base, c.src_off), addrs(base, c.rep_off)
    st, rec = np.full(1, 0xEE, np.uint8), np.full(2, 0xEEEE, np.uint64)
    rc = lib.fecgpu_block_svc_rlc_decode_rows(svc, ptr(rows), ptr(c.src_len), ptr(reps), ptr(c.rep_len), c.B, c.k, c.r,
                                              ptr(c.seeds), ptr(c.sp), ptr(c.rp), full, ptr(st), ptr(rec))
    return rc, int(st[0]), rec


def _patterns(rng, k, r):
    """(missing sources, repairs received): 0, 1 and min(k, r) erasures with enough repairs, and one erasure
    more than the received repairs allow."""
    em = min(k, r)
    out = []
    for e in sorted({0, 1, em}):
        p = int(rng.integers(e, r + 1))
        out.append((rng.choice(k, e, replace=False), rng.choice(r, p, replace=False)))
    out.append((rng.choice(k, em, replace=False), rng.choice(r, em - 1, replace=False)))
    return out


@pytest.mark.parametrize("k,r,B", [s for s in SHAPES if min(s[0], s[1]) <= 16])
def test_rlc_decode_matches_the_oracle(lib, svc, oracle, k, r, B):
    rng = np.random.default_rng(7 * k + r + B)
    seen = set()
    for x, (miss, present) in enumerate(_patterns(rng, k, r)):
        c = DecCase(oracle, k, r, B, miss, present, 1000 * k + 10 * B + x)
        pin = Pinned(lib, c.image)
        rc, st, rec = svc_decode(lib, svc, c, pin.base)
        assert rc == OK, lib.fecgpu_last_error()
        c.check(pin.h, st, rec, c.st, c.out, (k, r, B, x))
        for j, row in c.out.items():
            assert np.array_equal(row, c.padded[j])
        seen.add(c.st)
    assert DEC_NOTHING in seen and (DEC_RECOVERED in seen or k == 1)


def _full_rank_blocks():
    """Blocks of decode_full_cases' first tuple (k16 r4, 4 erasures, 4 repairs): one the reference
    elimination gives up on though its repairs determine it, one they do not determine, one it recovers."""
    c = case(*TUPLES[0], 64)
    give_up = int(np.nonzero((c.ref_st == REF_UB) & c.full)[0][0])
    singular = int(np.nonzero(~c.full)[0][0])
    ref_ok = int(np.nonzero(c.ref_st == RECOVERED)[0][0])
    return c, (give_up, singular, ref_ok)


def test_rlc_decode_full_mode_matches_the_launch_form(lib, svc, eng, oracle):
    c0, blocks = _full_rank_blocks()
    B = 61
    for b, want_full in zip(blocks, (RECOVERED, SINGULAR, RECOVERED)):
        c = DecCase(oracle, c0.k, c0.r, B, c0.miss[b], c0.present[b], 50 + b, fbn=b, src=c0.src[b])
        # reference mode on the same block, as the oracle has it
        pin = Pinned(lib, c.image)
        rc, st, rec = svc_decode(lib, svc, c, pin.base, full=0)
        assert rc == OK and st == c.st == int(c0.ref_st[b])
        c.check(pin.h, st, rec, c.st, c.out, ("ref", b))
        # full mode: the launch form on the same tables, in device memory
        pool = to_dev(c.image)
        st_d = torch.full((1,), 0xEE, dtype=torch.uint8, device=DEV)
        rec_d = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        ws = eng.alloc_workspace(1, c.k, c.r)
        t = [to_dev(a) for a in (addrs(pool.data_ptr(), c.src_off), c.src_len, addrs(pool.data_ptr(), c.rep_off),
                                 c.rep_len, np.array([B], np.uint32), c.seeds, c.sp, c.rp)]  # alive until the sync
        assert lib.fecgpu_rlc_decode_rows_fused_full(
            t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), 1, c.k, c.r, 64,
            t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), st_d.data_ptr(), rec_d.data_ptr(), ws.data_ptr(),
            ws.numel(), None) == OK
        torch.cuda.synchronize()
        assert int(st_d.cpu()[0]) == want_full
        pin = Pinned(lib, c.image)
        rc, st, rec = svc_decode(lib, svc, c, pin.base, full=1)
        assert rc == OK and st == want_full
        assert np.array_equal(rec, rec_d.cpu().numpy().view(np.uint64))
        if want_full == RECOVERED:
            out = {j: c.padded[j] for j in bits(rec, c.k)}
            assert sorted(out) == [j for j in c.miss if c.padded[j].any()]
            c.check(pin.h, st, rec, RECOVERED, out, ("full", b))
            assert np.array_equal(pin.h, pool.cpu().numpy())
        else:
            assert not rec.any() and np.array_equal(pin.h, c.image)  # SINGULAR: no row touched


# ------------------------------------------------------------------------------------------ XOR
@pytest.mark.parametrize("k", [1, 2, 4, 17, 100])
@pytest.mark.parametrize("B", [1, 19, 1200])
def test_xor_encode_matches_the_oracle(lib, svc, oracle, k, B):
    c = EncCase(oracle, k, 1, B, 31 * k + B, xor=True)
    pin = Pinned(lib, c.image)
    rows = addrs(pin.base, c.src_off)
    assert lib.fecgpu_block_svc_xor_encode_rows(svc, ptr(rows), ptr(c.src_len), pin.base + c.rep_off[0], B, k) == OK
    assert np.array_equal(pin.h, c.want), (k, B, np.flatnonzero(pin.h != c.want)[:8])


class XorDecCase:
    def __init__(self, oracle, k, B, miss, rep_present, seed):
        rng = np.random.default_rng(seed)
        self.k, self.B, self.miss = k, B, sorted(miss)
        lens = ragged(rng, k, B)
        padded = []
        for n in lens:
            row = np.zeros(B, np.uint8)
            row[:n] = rng.integers(0, 256, n, dtype=np.uint8)
            padded.append(row)
        ret, rep = oracle.xor_encode_block(padded)
        assert ret == 0 and len(rep) == B
        got = [j for j in range(k) if j not in self.miss]
        self.long = got[0] if got else None
        p = Pool()
        self.src_off, given = [], []
        self.src_len = np.zeros(k, np.uint32)
        for j in range(k):
            if j in self.miss:
                self.src_off.append(p.add(B))
                given.append(None)
                self.src_len[j] = 0xDEAD
                continue
            data = padded[j][:lens[j]]
            if j == self.long:  # longer than the block: truncated (xor_fec_scheme.c:54-70)
                data = np.concatenate([padded[j], rng.integers(1, 256, 5, dtype=np.uint8)])
            self.src_len[j] = len(data)
            self.src_off.append(p.add(len(data)) if len(data) else None)
            given.append(data)
        self.rep_off = p.add(B) if rep_present else None
        self.image = p.image()
        for o, d in zip(self.src_off, given):
            if d is not None and len(d):
                self.image[o:o + len(d)] = d
        if rep_present:
            self.image[self.rep_off:self.rep_off + B] = rep
        self.sp, self.rp = mask(got), mask([0] if rep_present else [])
        self.st, self.out = oracle.xor_decode_block(given, [rep if rep_present else None])
        self.want = self.image.copy()
        for j, row in self.out.items():
            assert np.array_equal(row, padded[j])
            self.want[self.src_off[j]:self.src_off[j] + B] = row


@pytest.mark.parametrize("k", [1, 2, 4, 17, 100])
@pytest.mark.parametrize("B", [1, 19, 1200])
def test_xor_decode_matches_the_oracle_and_the_launch_form(lib, svc, eng, oracle, k, B):
    rng = np.random.default_rng(17 * k + B)
    j = int(rng.integers(0, k))
    # REF_UB: every source received and no repair -- the count the reference checks holds (:45-49) and it
    # dereferences the missing repair
    cases = [([j], True, DEC_RECOVERED), ([], False, DEC_REF_UB), ([], True, DEC_NOTHING), ([j], False, DEC_NOTHING)]
    if k > 1:
        cases.append(([j, (j + 1) % k], True, DEC_NOTHING))
    for x, (miss, rep_present, want_st) in enumerate(cases):
        c = XorDecCase(oracle, k, B, miss, rep_present, 500 * k + B + x)
        # (without its repair the oracle's block form stops where xor_fec_scheme.c:50 would dereference NULL;
        # REF_UB is the engine's name for that pattern, by fecgpu_xor_decode_rows's rule)
        assert c.st == want_st or (not rep_present and c.out == {})
        pin = Pinned(lib, c.image)
        rows = addrs(pin.base, c.src_off)
        st, rec = np.full(1, 0xEE, np.uint8), np.full(2, 0xEEEE, np.uint64)
        assert lib.fecgpu_block_svc_xor_decode_rows(svc, ptr(rows), ptr(c.src_len),
                                                    0 if c.rep_off is None else pin.base + c.rep_off, B, k, ptr(c.sp),
                                                    ptr(c.rp), ptr(st), ptr(rec)) == OK
        assert st[0] == want_st and bits(rec, k) == sorted(c.out)
        assert np.array_equal(pin.h, c.want), (k, B, x, np.flatnonzero(pin.h != c.want)[:8])
        # fecgpu_xor_decode_rows on the same tables, in device memory
        pool = to_dev(c.image)
        st_d = torch.full((1,), 0xEE, dtype=torch.uint8, device=DEV)
        rec_d = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        rep_row = np.array([0 if c.rep_off is None else pool.data_ptr() + c.rep_off], np.uint64)
        eng.xor_decode_rows(to_dev(addrs(pool.data_ptr(), c.src_off)), to_dev(c.src_len), to_dev(rep_row),
                            to_dev(np.array([B], np.uint32)), to_dev(c.sp), to_dev(c.rp), st_d, rec_d, 1, k, (B + 3) & ~3)
        torch.cuda.synchronize()
        assert int(st_d.cpu()[0]) == st[0]
        assert np.array_equal(rec_d.cpu().numpy().view(np.uint64), rec)
        assert np.array_equal(pool.cpu().numpy(), pin.h)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_row_untouched(lib, svc, oracle):
    def refused(c, call):
        pin = Pinned(lib, c.image)
        assert call(c, pin.base) == ERR_INVALID
        assert np.array_equal(pin.h, c.image)

    # 17 unknowns: more than the worker solves
    rng = np.random.default_rng(3)
    c = DecCase(oracle, 20, 17, 37, rng.choice(20, 17, replace=False), range(17), 1)
    refused(c, lambda c, base: svc_decode(lib, svc, c, base)[0])
    # rows beyond the worker's LDS
    refused(EncCase(oracle, 64, 16, 9000, 2), lambda c, base: svc_encode(lib, svc, c, base))
    # a misaligned address: a source, then a repair
    c = EncCase(oracle, 5, 3, 19, 3)
    full = c.lens.index(19)

    def shifted(which):
        def call(c, base):
            rows, reps = addrs(base, c.src_off), addrs(base, c.rep_off)
            (rows if which == "src" else reps)[full if which == "src" else 1] += 2
            return lib.fecgpu_block_svc_rlc_encode_rows(svc, ptr(rows), ptr(c.src_len), ptr(reps), c.B, c.k, c.r, c.fbn)
        return call
    refused(c, shifted("src"))
    assert b"aligned" in lib.fecgpu_last_error()
    refused(c, shifted("rep"))
    # an address at 2^48
    def high(c, base):
        rows, reps = addrs(base, c.src_off), addrs(base, c.rep_off)
        reps[0] = 1 << 48
        return lib.fecgpu_block_svc_rlc_encode_rows(svc, ptr(rows), ptr(c.src_len), ptr(reps), c.B, c.k, c.r, c.fbn)
    refused(c, high)
    # src_len > blk_len
    def long_source(c, base):
        n = c.src_len.copy()
        n[full] = 20
        return lib.fecgpu_block_svc_rlc_encode_rows(svc, ptr(addrs(base, c.src_off)), ptr(n),
                                                    ptr(addrs(base, c.rep_off)), c.B, c.k, c.r, c.fbn)
    refused(c, long_source)
    assert b"src_len" in lib.fecgpu_last_error()
    x = EncCase(oracle, 4, 1, 19, 4, xor=True)
    def long_source_xor(c, base):
        n = c.src_len.copy()
        n[c.lens.index(19)] = 20
        return lib.fecgpu_block_svc_xor_encode_rows(svc, ptr(addrs(base, c.src_off)), ptr(n), base + c.rep_off[0], c.B,
                                                    c.k)
    refused(x, long_source_xor)
    # shapes
    for k, r, B in ((0, 3, 19), (129, 3, 19), (5, 0, 19), (5, 129, 19), (5, 3, 0), (5, 3, 65533)):
        refused(c, lambda c, base: lib.fecgpu_block_svc_rlc_encode_rows(
            svc, ptr(addrs(base, c.src_off)), ptr(c.src_len), ptr(addrs(base, c.rep_off)), B, k, r, c.fbn))
    # knob block_svc 0: every kind is refused; restored afterwards
    assert lib.fecgpu_set_knob(b"block_svc", 0) == 0
    try:
        refused(c, lambda c, base: svc_encode(lib, svc, c, base))
        refused(x, lambda c, base: lib.fecgpu_block_svc_xor_encode_rows(
            svc, ptr(addrs(base, c.src_off)), ptr(c.src_len), base + c.rep_off[0], c.B, c.k))
    finally:
        assert lib.fecgpu_set_knob(b"block_svc", 1) == 0
    pin = Pinned(lib, c.image)
    assert svc_encode(lib, svc, c, pin.base) == OK  # and served again
    assert np.array_equal(pin.h, c.want)


# ------------------------------------------------------------------------------------------ mixed requests
def test_packed_and_row_requests_alternate_on_one_service(lib, svc, oracle):
    k, r, L = 16, 4, 1200
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (1, k, L), dtype=np.uint8)
    ts = torch.from_numpy(src).pin_memory()
    tr = torch.zeros((1, r, L), dtype=torch.uint8).pin_memory()
    want_packed = oracle.rlc_encode_batch(src, r, 77)
    # the packed decode: sources 3 and 9 missing, every repair received
    miss = [3, 9]
    work = src.copy()
    work[0, miss] = 0
    seeds = np.array([(77 << 8) | i for i in range(r)], np.uint32)
    sp, rp = mask([j for j in range(k) if j not in miss]), mask(range(r))
    trep = torch.from_numpy(want_packed.copy()).pin_memory()
    enc = EncCase(oracle, 16, 4, 1198, 21)
    xdec = XorDecCase(oracle, 17, 19, [5], True, 22)
    for it in range(20):
        tr.zero_()
        assert lib.fecgpu_block_svc_rlc_encode(svc, ts.data_ptr(), tr.data_ptr(), k, r, L, 77) == OK
        assert np.array_equal(tr.numpy(), want_packed), it
        pin = Pinned(lib, enc.image)
        assert svc_encode(lib, svc, enc, pin.base) == OK
        assert np.array_equal(pin.h, enc.want), it
        pin = Pinned(lib, xdec.image)
        st, rec = np.full(1, 0xEE, np.uint8), np.full(2, 0xEEEE, np.uint64)
        assert lib.fecgpu_block_svc_xor_decode_rows(svc, ptr(addrs(pin.base, xdec.src_off)), ptr(xdec.src_len),
                                                    pin.base + xdec.rep_off, xdec.B, xdec.k, ptr(xdec.sp), ptr(xdec.rp),
                                                    ptr(st), ptr(rec)) == OK
        assert st[0] == DEC_RECOVERED and bits(rec, xdec.k) == [5] and np.array_equal(pin.h, xdec.want), it
        tw = torch.from_numpy(work.copy()).pin_memory()
        st, rec = np.full(1, 0xEE, np.uint8), np.full(2, 0xEEEE, np.uint64)
        assert lib.fecgpu_block_svc_rlc_decode_seeded(svc, tw.data_ptr(), trep.data_ptr(), tw.data_ptr(), k, r, L,
                                                      ptr(seeds), ptr(sp), ptr(rp), ptr(st), ptr(rec)) == OK
        assert st[0] == DEC_RECOVERED and bits(rec, k) == miss and np.array_equal(tw.numpy(), src), it
