"""XOR on rows (fecgpu_xor_encode_rows / fecgpu_xor_decode_rows and their host forms) against the CPU
oracle's per-block, per-length XOR encode and decode.  Byte work: every comparison is exact.  Rows live in
one pool at 4-byte aligned offsets that are never 16-byte aligned, with 0xA5 guard bytes between them,
and after each call the whole pool image is compared with the expected one: sources untouched, outputs
exactly blk_len bytes, guards intact.  Every address handed to a kernel comes from a live allocation
(or is 0 where the interface says the row is never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import DEC_NOTHING, DEC_RECOVERED, DEC_REF_UB, Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
GUARD = 0xA5
# k, symbol_size, nblocks
SHAPES = [(1, 4, 1), (2, 16, 3), (3, 36, 5), (5, 1200, 67), (16, 1200, 257), (17, 1500, 33), (100, 64, 9),
          (128, 20, 4), (4, 9000, 3)]


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(0)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def to_dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Pool:
    """Rows in one byte pool: row q starts at offset 4, 8 or 12 mod 16 (by turns) and is followed by at
    least 20 guard bytes."""

    def __init__(self):
        self.end, self.n = 64, 0

    def add(self, room):
        o = ((self.end + 15) & ~15) + 4 * (1 + self.n % 3)
        self.n += 1
        self.end = o + room + 20
        return o

    def image(self):
        return np.full(self.end + 64, GUARD, np.uint8)


def _lengths(rng, b, k, S):
    cand = sorted({min(max(x, 0), S) for x in (0, 1, 2, 3, 4, 5, 15, 16, 17, S - 1, S)})
    lens = [cand[(b * k + j) % len(cand)] if rng.random() < 0.5 else int(rng.integers(0, S + 1)) for j in range(k)]
    if b % 5 == 0:
        lens[b % k] = S
    return lens


def _addr(base, off):
    """Table of addresses: base + offset, 0 where the row has none."""
    return np.array([0 if o is None else base + o for o in off], np.uint64)


# ---------------------------------------------------------------------------------- encode
class EncodeCase:
    """nb ragged blocks plus two special ones: every source empty under a block length of 8 (the repair is
    zeros), and a block of length 0 with all its addresses 0."""

    def __init__(self, oracle, k, S, nb, seed, equal=False):
        rng = np.random.default_rng(seed)
        p = Pool()
        self.k, self.S = k, S
        lens = [[S] * k if equal else _lengths(rng, b, k, S) for b in range(nb)]
        blk = [max(x) for x in lens]
        if not equal:
            lens += [[0] * k, [0] * k]
            blk += [min(8, S), 0]
        self.nb = len(lens)
        self.src_off, self.rep_off = [], []
        for b in range(self.nb):
            self.src_off += [p.add(n) if n else None for n in lens[b]]
            self.rep_off.append(p.add(blk[b]) if blk[b] else None)
        self.src_len = np.array(lens, np.uint32).reshape(-1)
        self.blk_len = np.array(blk, np.uint32)
        self.image = p.image()
        self.srcs = []
        for b in range(self.nb):
            row = []
            for j in range(k):
                n, o = lens[b][j], self.src_off[b * k + j]
                d = rng.integers(0, 256, n, dtype=np.uint8)
                if n:
                    self.image[o:o + n] = d
                row.append(d)
            self.srcs.append(row)
        self.want = self.image.copy()
        for b in range(self.nb):
            if not blk[b]:
                continue
            if max(lens[b]) == 0:
                rep = np.zeros(blk[b], np.uint8)
            else:
                ret, rep = oracle.xor_encode_block(self.srcs[b])
                assert ret == 0 and len(rep) == blk[b]
            self.want[self.rep_off[b]:self.rep_off[b] + blk[b]] = rep

    def tables(self, base):
        return _addr(base, self.src_off), _addr(base, self.rep_off)


@pytest.mark.parametrize("k,S,nb", SHAPES)
def test_encode_matches_the_oracle(eng, oracle, k, S, nb):
    c = EncodeCase(oracle, k, S, nb, 1000 * k + S + nb)
    pool = to_dev(c.image)
    rows, reps = c.tables(pool.data_ptr())
    given_src, given_blk = c.src_len.copy(), c.blk_len.copy()
    # the kernels clamp: a block length above symbol_size, a source length above the block's
    full = np.flatnonzero(c.blk_len == S)
    if len(full):
        given_blk[full[0]] = S + 100
    at_blk = [x for x in range(c.nb * k) if c.src_len[x] and c.src_len[x] == c.blk_len[x // k] and x // k not in full[:1]]
    if at_blk:
        given_src[at_blk[0]] += 50
    eng.xor_encode_rows(to_dev(rows), to_dev(given_src), to_dev(reps), to_dev(given_blk), c.nb, k, S)
    torch.cuda.synchronize()
    got = pool.cpu().numpy()
    assert np.array_equal(got, c.want), (k, S, nb, np.flatnonzero(got != c.want)[:8])


@pytest.mark.parametrize("k,S,nb", [(5, 1200, 67), (16, 1200, 257), (17, 1500, 33), (128, 20, 4)])
def test_equal_lengths_match_the_packed_kernel(eng, oracle, k, S, nb):
    c = EncodeCase(oracle, k, S, nb, 7 * k + S, equal=True)
    pool = to_dev(c.image)
    rows, reps = c.tables(pool.data_ptr())
    eng.xor_encode_rows(to_dev(rows), to_dev(c.src_len), to_dev(reps), to_dev(c.blk_len), nb, k, S)
    packed = to_dev(np.stack([np.stack(r) for r in c.srcs]))
    rep = torch.empty((nb, 1, S), dtype=torch.uint8, device=DEV)
    eng.xor_encode(packed, rep, k, S)
    torch.cuda.synchronize()
    got, rep_h = pool.cpu().numpy(), rep.cpu().numpy()
    assert np.array_equal(got, c.want)
    for b in range(nb):
        assert np.array_equal(got[c.rep_off[b]:c.rep_off[b] + S], rep_h[b, 0]), b


# ---------------------------------------------------------------------------------- decode
class DecodeCase:
    """Blocks by turns: one source missing (index 0, k - 1, a middle one -- 70 when k = 100), two missing
    (NOTHING), none missing with the repair (NOTHING), all present without the repair (REF_UB).  Some
    received sources are longer than the block (truncated; longer=False leaves them out: the host forms
    refuse them); mask bits above k are set."""

    def __init__(self, oracle, k, S, nb, seed, longer=True):
        rng = np.random.default_rng(seed)
        p = Pool()
        self.k, self.S, self.nb = k, S, nb
        self.src_off, self.rep_off = [], []
        src_len, blk_len = [], []
        self.sp, self.rp = np.zeros((nb, 2), np.uint64), np.zeros((nb, 2), np.uint64)
        self.st = np.zeros(nb, np.uint8)
        self.rec = np.zeros((nb, 2), np.uint64)
        fills, outs = [], []
        for b in range(nb):
            lens = _lengths(rng, b, k, S)
            if b % 3 == 1:  # a block shorter than the symbol size: room for a received source longer than it
                lens = [min(n, max(S - 8, 1)) for n in lens]
            full = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
            blk = max(lens)
            repair = oracle.xor_encode_block(full)[1] if blk else np.zeros(0, np.uint8)
            turn = b % 6 if k > 1 else (0, 4, 5)[b % 3]
            miss = {0: [0], 1: [k - 1], 2: [70 if k > 70 else k // 2], 3: [0, k - 1], 4: [], 5: []}[turn]
            have_rep = turn != 5
            recv = [None if j in miss else full[j] for j in range(k)]
            if longer and blk and blk < S:  # a received source longer than the block: read for blk bytes only
                for j in range(k):
                    if recv[j] is not None:
                        extra = rng.integers(1, 256, min(S, blk + 7) - blk, dtype=np.uint8)
                        recv[j] = np.concatenate([recv[j], np.zeros(blk - len(recv[j]), np.uint8), extra])
                        break
            st, want = oracle.xor_decode_block(recv, [repair if have_rep else None])
            assert st == {0: DEC_RECOVERED, 1: DEC_RECOVERED, 2: DEC_RECOVERED, 3: DEC_NOTHING, 4: DEC_NOTHING,
                          5: DEC_REF_UB}[turn]
            self.st[b] = st
            for j in range(k):
                if recv[j] is not None:
                    self.sp[b, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
                    o = p.add(len(recv[j])) if len(recv[j]) else None
                    fills.append((o, recv[j]))
                else:  # the row the recovered bytes go to (untouched unless the block is RECOVERED)
                    o = p.add(blk) if blk else None
                src_len.append(0 if recv[j] is None else len(recv[j]))
                self.src_off.append(o)
            if k < 128:  # bits above k are ignored
                self.sp[b, k >> 6] |= np.uint64((1 << 64) - (1 << (k & 63)))
                if k < 64:
                    self.sp[b, 1] = np.uint64(2 ** 64 - 1)
            self.rp[b, 0] = np.uint64(0xFFFE | int(have_rep))
            self.rp[b, 1] = np.uint64(7)
            ro = p.add(blk) if have_rep and blk else None
            if ro is not None:
                fills.append((ro, repair))
            self.rep_off.append(ro)
            blk_len.append(blk)
            for j, v in want.items():
                assert len(v) == blk and np.array_equal(v[:len(full[j])], full[j]) and not v[len(full[j]):].any()
                self.rec[b, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
                if blk:
                    outs.append((self.src_off[b * k + j], v))
        self.src_len, self.blk_len = np.array(src_len, np.uint32), np.array(blk_len, np.uint32)
        self.image = p.image()
        for o, d in fills:
            if o is not None:
                self.image[o:o + len(d)] = d
        self.want = self.image.copy()
        for o, d in outs:
            self.want[o:o + len(d)] = d

    def tables(self, base):
        return _addr(base, self.src_off), _addr(base, self.rep_off)


def _decode_dev(eng, c):
    pool = to_dev(c.image)
    rows, reps = c.tables(pool.data_ptr())
    st = torch.full((c.nb,), 0xEE, dtype=torch.uint8, device=DEV)
    rec = torch.full((c.nb, 2), -1, dtype=torch.int64, device=DEV)
    eng.xor_decode_rows(to_dev(rows), to_dev(c.src_len), to_dev(reps), to_dev(c.blk_len), to_dev(c.sp), to_dev(c.rp),
                        st, rec, c.nb, c.k, c.S)
    torch.cuda.synchronize()
    return pool.cpu().numpy(), st.cpu().numpy(), rec.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("k,S,nb", [(1, 4, 3), (2, 16, 7), (3, 36, 13), (5, 1200, 67), (16, 1200, 131), (17, 1500, 33),
                                    (100, 64, 13), (128, 20, 7), (4, 9000, 6)])
def test_decode_matches_the_oracle(eng, oracle, k, S, nb):
    c = DecodeCase(oracle, k, S, nb, 31 * k + S + nb)
    assert {DEC_RECOVERED, DEC_NOTHING, DEC_REF_UB} <= set(c.st.tolist())
    got, st, rec = _decode_dev(eng, c)
    assert np.array_equal(st, c.st), (st, c.st)
    assert np.array_equal(rec, c.rec)
    assert np.array_equal(got, c.want), (k, S, nb, np.flatnonzero(got != c.want)[:8])


def test_decode_missing_index_above_64(eng, oracle):
    c = DecodeCase(oracle, 100, 64, 13, 5)
    assert int(c.rec[2, 1]) == 1 << (70 - 64) and int(c.rec[2, 0]) == 0
    got, st, rec = _decode_dev(eng, c)
    assert np.array_equal(rec, c.rec) and np.array_equal(got, c.want)


# ---------------------------------------------------------------------------------- host forms
class HostMem:
    """Arrays in page-locked memory (fecgpu_host_alloc) or pageable numpy arrays."""

    def __init__(self, lib, pinned):
        self.lib, self.pinned, self.keep = lib, pinned, []
        lib.fecgpu_host_alloc.restype = C.c_void_p
        lib.fecgpu_host_alloc.argtypes = [C.c_size_t]
        lib.fecgpu_host_free.argtypes = [C.c_void_p]

    def array(self, a, pinned=None):
        a = np.ascontiguousarray(a)
        if not (self.pinned if pinned is None else pinned):
            return a.copy()
        p = self.lib.fecgpu_host_alloc(max(a.nbytes, 16))
        assert p
        self.keep.append(p)
        out = np.frombuffer((C.c_uint8 * max(a.nbytes, 16)).from_address(p), np.uint8)[:a.nbytes].view(a.dtype)
        out = out.reshape(a.shape)
        out[...] = a
        return out

    def close(self):
        for p in self.keep:
            self.lib.fecgpu_host_free(p)
        self.keep = []


def _dev_addr(lib, a):
    d = C.c_uint64(0)
    assert lib.fecgpu_host_device_address(a.ctypes.data, a.nbytes, C.byref(d)) == 0
    return d.value


@pytest.fixture(scope="module")
def hostpath(eng):
    from pquic_amd.engine import HostPath
    hp = HostPath(0, nstreams=3, chunk_bytes=64 << 10)  # about 10 blocks of k4 L1200 per sub-batch
    yield hp
    hp.close()


@pytest.fixture(scope="module")
def host_cases(oracle):
    return EncodeCase(oracle, 4, 1200, 298, 77), DecodeCase(oracle, 4, 1200, 300, 78, longer=False)


@pytest.mark.parametrize("pinned", [False, True])
def test_host_forms(eng, hostpath, host_cases, pinned):
    """300 blocks over several sub-batches, rows in fecgpu_host_alloc memory, tables pageable or page-locked:
    the same bytes, status and masks as the device form (and the oracle)."""
    enc, dec = host_cases
    hm = HostMem(eng.lib, pinned)
    try:
        pool = hm.array(enc.image, pinned=True)
        rows, reps = enc.tables(_dev_addr(eng.lib, pool))
        hostpath.xor_encode_rows(hm.array(rows), hm.array(enc.src_len), hm.array(reps), hm.array(enc.blk_len),
                                 enc.nb, enc.k, enc.S)
        assert np.array_equal(pool, enc.want), np.flatnonzero(pool != enc.want)[:8]

        dev_pool, dev_st, dev_rec = _decode_dev(eng, dec)
        pool = hm.array(dec.image, pinned=True)
        rows, reps = dec.tables(_dev_addr(eng.lib, pool))
        st = hm.array(np.full(dec.nb, 0xEE, np.uint8))
        rec = hm.array(np.full((dec.nb, 2), 2 ** 64 - 1, np.uint64))
        hostpath.xor_decode_rows(hm.array(rows), hm.array(dec.src_len), hm.array(reps), hm.array(dec.blk_len),
                                 hm.array(dec.sp), hm.array(dec.rp), st, rec, dec.nb, dec.k, dec.S)
        assert np.array_equal(st, dev_st) and np.array_equal(st, dec.st)
        assert np.array_equal(rec, dev_rec) and np.array_equal(rec, dec.rec)
        assert np.array_equal(pool, dev_pool) and np.array_equal(pool, dec.want)
    finally:
        hm.close()


# ---------------------------------------------------------------------------------- round trip
def test_round_trip_on_device_tensors(eng):
    nb, k, L = 1 << 14, 4, 1200
    g = torch.Generator(device=DEV).manual_seed(9)
    src = torch.randint(0, 256, (nb, k, L), dtype=torch.uint8, device=DEV, generator=g)
    rep = torch.full((nb, L), GUARD, dtype=torch.uint8, device=DEV)
    rows = src.data_ptr() + torch.arange(nb * k, dtype=torch.int64, device=DEV) * L
    reps = rep.data_ptr() + torch.arange(nb, dtype=torch.int64, device=DEV) * L
    src_len = torch.full((nb * k,), L, dtype=torch.int32, device=DEV)
    blk_len = torch.full((nb,), L, dtype=torch.int32, device=DEV)
    eng.xor_encode_rows(rows, src_len, reps, blk_len, nb, k, L)
    orig = src.clone()
    miss = torch.arange(nb, device=DEV) % k  # one source of every block is dropped
    src[torch.arange(nb, device=DEV), miss] = GUARD
    sp = torch.zeros((nb, 2), dtype=torch.int64, device=DEV)
    sp[:, 0] = ((1 << k) - 1) & ~(1 << miss)
    rp = torch.zeros((nb, 2), dtype=torch.int64, device=DEV)
    rp[:, 0] = 1
    st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
    rec = torch.zeros((nb, 2), dtype=torch.int64, device=DEV)
    eng.xor_decode_rows(rows, src_len, reps, blk_len, sp, rp, st, rec, nb, k, L)
    torch.cuda.synchronize()
    assert int(st.max()) == DEC_RECOVERED
    assert torch.equal(rec[:, 0], 1 << miss) and not bool(rec[:, 1].any())
    assert torch.equal(src, orig)
