"""Ragged rows on the device: the gather / scatter primitives, fecgpu_rlc_encode_rows_len and
fecgpu_rlc_decode_rows_len and their host forms, against the reference's own ragged fixtures and the CPU
oracle's per-block, per-length encode and decode.  Byte work: every comparison is exact, and every
output is compared as the whole pool the rows live in, so a byte written past a row's length -- in the
dword that holds its last byte, in the gap behind it or in the row that follows -- fails the test."""
import ctypes as C

import numpy as np
import pytest

from golden_io import decode_sources, load
from oracle_py import DEC_RECOVERED, Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = 0xC3
ERR_INVALID = -1
SEED = 20261019
SHAPES = [(1, 1), (2, 1), (4, 2), (16, 4), (32, 8), (64, 16)]
NBLOCKS = (1, 3, 65, 129)


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


def pad4(n):
    return (n + 3) & ~3


def bits(m, n):
    return [j for j in range(n) if (int(m[j >> 6]) >> (j & 63)) & 1]


def mask(present, n):
    m = np.zeros(2, np.uint64)
    for j in range(n):
        if present[j]:
            m[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return m


class Pool:
    """Rows of their own length in one byte pool: row q starts 4-byte aligned at offset 0, 4, 8 or 12
    mod 16 (by turns), and a gap of canary bytes follows every row."""

    def __init__(self, room):
        self.off = []
        self.end = 64
        self.room = room  # bytes kept for every row, whatever its length

    def add(self, n=None):
        n = self.room if n is None else n
        q = len(self.off)
        base = (self.end + 15) & ~15
        o = base + 4 * ((q % 17 + q // 17) % 4)  # the turn shifts every 17 rows: every length meets every offset
        self.off.append(o)
        self.end = o + n + 20
        return o

    def bytes(self):
        return np.full(self.end + 64, CANARY, np.uint8)


# ---------------------------------------------------------------------------------- primitives
LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def _lens_for(L, nrows):
    cand = [min(x, L) for x in LENS + (L - 1, L)]
    # row x takes the length of turn x mod 17 and the offset of turn (x mod 17 + x // 17) mod 4 (Pool.add):
    # with 257 rows every length meets every alignment
    return np.array([cand[x % len(cand)] for x in range(nrows)], np.uint32)


def _pool_rows(L, nrows):
    p = Pool(L)
    return p, np.array([p.add() for _ in range(nrows)], np.int64)


@pytest.mark.parametrize("L", [4, 8, 36, 1200, 2052])
def test_gather_exact_bytes_then_zeros(eng, L):
    rng = np.random.default_rng(L)
    for nrows in (1, 63, 65, 257):
        lens = _lens_for(L, nrows)
        p, off = _pool_rows(L, nrows)
        assert {int(o) % 16 for o in off} == ({0, 4, 8, 12} if nrows > 4 else {int(off[0]) % 16})
        if nrows == 257:
            assert len({(int(n), int(o) % 16) for n, o in zip(lens, off)}) == 4 * len(set(lens.tolist()))
        pool_h = rng.integers(1, 256, p.end + 64, dtype=np.uint8)
        pool = to_dev(pool_h)
        rows = (pool.data_ptr() + off).astype(np.uint64)
        rows[lens == 0] = 0  # never dereferenced
        given = lens.copy()
        if nrows > 1:  # a length above symbol_size is clamped (the pool holds L bytes of the row)
            given[np.flatnonzero(lens == L)[0]] = L + 100
        dst = torch.full((nrows + 1, L), CANARY, dtype=torch.uint8, device=DEV)
        d_rows, d_len = to_dev(rows), to_dev(given)
        eng.rows_gather(d_rows, d_len, nrows, L, dst)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        want = np.zeros((nrows + 1, L), np.uint8)
        want[nrows] = CANARY  # the row after the batch
        for x in range(nrows):
            want[x, :lens[x]] = pool_h[off[x]:off[x] + lens[x]]
        assert np.array_equal(got, want), (L, nrows, np.argwhere(got != want)[:4])
        assert np.array_equal(pool.cpu().numpy(), pool_h)


@pytest.mark.parametrize("L", [4, 8, 36, 1200, 2052])
def test_scatter_writes_len_bytes_and_not_one_more(eng, L):
    rng = np.random.default_rng(L + 1)
    for nrows in (1, 63, 65, 257):
        lens = _lens_for(L, nrows)
        p, off = _pool_rows(L, nrows)
        pool = to_dev(p.bytes())
        rows = (pool.data_ptr() + off).astype(np.uint64)
        rows[lens == 0] = 0  # length 0 with address 0: accepted, touches nothing
        src_h = rng.integers(0, 256, (nrows, L), dtype=np.uint8)
        src = to_dev(src_h)
        d_rows, d_len = to_dev(rows), to_dev(lens)
        eng.rows_scatter(src, d_rows, d_len, nrows, L)
        torch.cuda.synchronize()
        want = p.bytes()
        for x in range(nrows):
            want[off[x]:off[x] + lens[x]] = src_h[x, :lens[x]]
        got = pool.cpu().numpy()
        assert np.array_equal(got, want), (L, nrows, np.flatnonzero(got != want)[:8])
        assert np.array_equal(src.cpu().numpy(), src_h)


def test_scatter_clamps_a_length_above_symbol_size(eng):
    L, nrows = 36, 5
    p, off = _pool_rows(L + 200, nrows)
    pool = to_dev(p.bytes())
    src_h = np.arange(nrows * L, dtype=np.uint32).astype(np.uint8).reshape(nrows, L) | 1
    src = to_dev(src_h)
    d_rows = to_dev((pool.data_ptr() + off).astype(np.uint64))
    d_len = to_dev(np.array([L + 1, L + 150, 7, 0, 1 << 31], np.uint32))
    eng.rows_scatter(src, d_rows, d_len, nrows, L)
    torch.cuda.synchronize()
    want = p.bytes()
    for x, n in enumerate((L, L, 7, 0, L)):
        want[off[x]:off[x] + n] = src_h[x, :n]
    assert np.array_equal(pool.cpu().numpy(), want)


# ---------------------------------------------------------------------------------- batches
class Ragged:
    """A ragged batch in a pool: sources and repairs of their own lengths, the tables that describe
    them, and (after expect_*) the pool the device must leave behind."""

    def __init__(self, rng, nb, k, r, L, decode=False):
        self.nb, self.k, self.r, self.L = nb, k, r, L
        blk = rng.integers(2, L + 1, nb).astype(np.uint32)
        if nb >= 3:
            blk[0], blk[1], blk[2] = (1 if decode else 0), 1, L  # (a decode block has at least one byte)
        self.blk = blk
        self.src_len = np.zeros((nb, k), np.uint32)
        self.src = np.zeros((nb, k, L), np.uint8)  # zero-padded
        for b in range(nb):
            n = rng.integers(0 if not decode else 1, int(blk[b]) + 1, k)
            if not decode and k > 2:
                n[rng.integers(0, k)] = 0  # some sources have no bytes
            n[rng.integers(0, k)] = blk[b]  # one source is as long as the block
            self.src_len[b] = n
            for j in range(k):
                self.src[b, j, :n[j]] = rng.integers(1, 256, int(n[j]), dtype=np.uint8)
        self.pool = Pool(None)
        # an encode source row holds its own bytes; a decode one may be recovered into: blk bytes
        self.src_off = np.array([[self.pool.add(int(blk[b] if decode else self.src_len[b, j])) for j in range(k)]
                                 for b in range(nb)], np.int64).reshape(nb, k)
        # repairs keep room for a longer (truncated) row; recovered sources are written for blk bytes
        self.rep_off = np.array([[self.pool.add(int(blk[b]) + 8) for _ in range(r)] for b in range(nb)],
                                np.int64).reshape(nb, r)

    def fill_sources(self, pool_h, present=None):
        for b in range(self.nb):
            for j in range(self.k):
                if present is None or present[b][j]:
                    n = int(self.src_len[b, j])
                    pool_h[self.src_off[b, j]:self.src_off[b, j] + n] = self.src[b, j, :n]


def encode_seeded(oracle, src, seeds):
    """Repairs of zero-padded blocks, repair i of block b seeded by seeds[b, i]."""
    nb, k, L = src.shape
    r = seeds.shape[1]
    mul, _ = oracle.gf_tables()
    rep = np.zeros((nb, r, L), np.uint8)
    for b in range(nb):
        for i in range(r):
            coef = oracle.coefs(int(seeds[b, i]), k)
            acc = rep[b, i]
            for j in range(k):
                acc ^= mul[coef[j]][src[b, j]]
    return rep


def _encode_case(rng, oracle, nb, k, r, L):
    g = Ragged(rng, nb, k, r, L)
    fbn = rng.integers(0, 1 << 24, nb).astype(np.uint32)
    pool_h = g.pool.bytes()
    g.fill_sources(pool_h)
    want = pool_h.copy()
    for b in range(nb):
        if g.blk[b] == 0:
            continue  # a block of no bytes: no repair row is touched
        ret, reps = oracle.rlc_encode_block(int(fbn[b]), [g.src[b, j, :g.src_len[b, j]] for j in range(k)], r)
        assert ret == 0 and all(len(x) == g.blk[b] for x in reps)
        for i in range(r):
            want[g.rep_off[b, i]:g.rep_off[b, i] + g.blk[b]] = reps[i]
    return g, fbn, pool_h, want


def _encode_tables(g, base):
    rows_s = (base + g.src_off.reshape(-1)).astype(np.uint64)
    rows_s[g.src_len.reshape(-1) == 0] = 0
    rows_r = (base + g.rep_off.reshape(-1)).astype(np.uint64)
    return rows_s, g.src_len.reshape(-1).copy(), rows_r, g.blk.copy()


@pytest.mark.parametrize("k,r", SHAPES)
def test_encode_ragged_vs_oracle(eng, oracle, k, r):
    rng = np.random.default_rng(SEED + 100 * k + r)
    for nb in NBLOCKS:
        g, fbn, pool_h, want = _encode_case(rng, oracle, nb, k, r, 1200)
        pool = to_dev(pool_h)
        t = [to_dev(x) for x in _encode_tables(g, pool.data_ptr())]
        d_fbn = to_dev(fbn)
        eng.rlc_encode_rows_len(t[0], t[1], t[2], t[3], nb, k, r, 1200, fbn=d_fbn)
        torch.cuda.synchronize()
        got = pool.cpu().numpy()
        assert np.array_equal(got, want), (k, r, nb, np.flatnonzero(got != want)[:8])


def test_encode_ragged_k64_r16_9000(eng, oracle):
    rng = np.random.default_rng(SEED + 9000)
    nb, k, r, L = 3, 64, 16, 9000
    g, fbn, pool_h, want = _encode_case(rng, oracle, nb, k, r, L)
    pool = to_dev(pool_h)
    t = [to_dev(x) for x in _encode_tables(g, pool.data_ptr())]
    d_fbn = to_dev(fbn)
    eng.rlc_encode_rows_len(t[0], t[1], t[2], t[3], nb, k, r, L, fbn=d_fbn)
    torch.cuda.synchronize()
    assert np.array_equal(pool.cpu().numpy(), want)


def test_encode_varlen_fixtures(eng):
    """Every ragged RLC case the reference recorded (encode_cases.json "varlen"), at the smallest stride
    that holds it and at a larger one: the recorded repair bytes, canaries behind them."""
    cases = [c for c in load("encode_cases.json")["varlen"] if c["scheme"] == "rlc" and c["ret"] == 0]
    assert cases
    for case in cases:
        srcs = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in case["src_hex"]]
        reps = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in case["rep_hex"]]
        k, r, maxl = len(srcs), case["r"], max(len(s) for s in srcs)
        for L in (max(pad4(maxl), 4), pad4(maxl) + 52):
            p = Pool(None)
            so = [p.add(len(s)) for s in srcs]
            ro = [p.add(maxl) for _ in range(r)]
            pool_h = p.bytes()
            for o, s in zip(so, srcs):
                pool_h[o:o + len(s)] = s
            want = pool_h.copy()
            for o, x in zip(ro, reps):
                assert len(x) == maxl
                want[o:o + maxl] = x
            pool = to_dev(pool_h)
            base = pool.data_ptr()
            d = [to_dev(np.array([base + o for o in so], np.uint64)), to_dev(np.array([len(s) for s in srcs], np.uint32)),
                 to_dev(np.array([base + o for o in ro], np.uint64)), to_dev(np.array([maxl], np.uint32))]
            eng.rlc_encode_rows_len(d[0], d[1], d[2], d[3], 1, k, r, L, fbn_base=case["fbn"])
            torch.cuda.synchronize()
            assert np.array_equal(pool.cpu().numpy(), want), (case.get("tag"), L)


@pytest.mark.parametrize("k,r,L,nb", [(16, 4, 1200, 129), (4, 2, 36, 65), (64, 16, 1200, 3)])
def test_encode_equal_lengths_match_encode_rows(eng, k, r, L, nb):
    rng = np.random.default_rng(SEED + k)
    src_h = rng.integers(0, 256, (nb, k, L), dtype=np.uint8)
    src = to_dev(src_h)
    reps = [torch.full((nb, r, L + 4), CANARY, dtype=torch.uint8, device=DEV) for _ in range(2)]
    rows_s = to_dev((src.data_ptr() + np.arange(nb * k, dtype=np.int64) * L).astype(np.uint64))
    d_sl = to_dev(np.full(nb * k, L, np.uint32))
    d_bl = to_dev(np.full(nb, L, np.uint32))
    rows_r = [to_dev((x.data_ptr() + np.arange(nb * r, dtype=np.int64) * (L + 4)).astype(np.uint64)) for x in reps]
    eng.rlc_encode_rows(rows_s, rows_r[0], nb, k, r, L, fbn_base=77)
    eng.rlc_encode_rows_len(rows_s, d_sl, rows_r[1], d_bl, nb, k, r, L, fbn_base=77)
    torch.cuda.synchronize()
    a, b = reps[0].cpu().numpy(), reps[1].cpu().numpy()
    assert np.array_equal(a, b) and (a[:, :, L:] == CANARY).all() and (a[:, :, :L] != CANARY).any()


# ---------------------------------------------------------------------------------- decode
class DecodeCase:
    """A ragged decode batch, the oracle's verdict on it, and the pool the device must leave."""

    def __init__(self, rng, oracle, nb, k, r, L):
        g = self.g = Ragged(rng, nb, k, r, L, decode=True)
        self.seeds = np.zeros((nb, r), np.uint32)
        for b in range(nb):
            for i in range(r):
                self.seeds[b, i] = ((int(rng.integers(0, 1 << 24)) << 8) | i) if b % 2 else int(rng.integers(0, 1 << 32))
        rep = encode_seeded(oracle, g.src, self.seeds)
        self.rep_len = np.repeat(g.blk[:, None], r, 1).astype(np.uint32)
        self.present = np.ones((nb, k), bool)
        zero_src = None
        for b in range(nb):
            e = int(rng.integers(1, min(k, r) + 1))
            self.present[b, rng.choice(k, e, replace=False)] = False
        if nb >= 3 and k >= 2:  # one missing source that is all zeros: determined, but its bit stays clear
            zero_src = (2, int(np.flatnonzero(~self.present[2])[0]))
            g.src[zero_src] = 0
            rep[2] = encode_seeded(oracle, g.src[2:3], self.seeds[2:3])[0]
        pool_h = g.pool.bytes()
        g.fill_sources(pool_h, self.present)
        long_rep = None
        for b in range(nb):
            for i in range(r):
                n = int(g.blk[b])
                pool_h[g.rep_off[b, i]:g.rep_off[b, i] + n] = rep[b, i, :n]
        if r >= 2:  # one repair longer than its block: read up to the block's length only
            long_rep = (nb - 1, r - 1)
            self.rep_len[long_rep] += 8
            o = g.rep_off[long_rep] + int(g.blk[nb - 1])
            pool_h[o:o + 8] = rng.integers(1, 256, 8, dtype=np.uint8)
        self.pool_h = pool_h
        self.want = pool_h.copy()
        self.status = np.zeros(nb, np.uint8)
        self.rec = np.zeros((nb, 2), np.uint64)
        self.sp = np.stack([mask(self.present[b], k) for b in range(nb)])
        self.rp = np.stack([mask([True] * r, r) for _ in range(nb)])
        self.n_recovered_blocks = 0
        for b in range(nb):
            srcs = [g.src[b, j, :g.src_len[b, j]] if self.present[b, j] else None for j in range(k)]
            reps = [pool_h[g.rep_off[b, i]:g.rep_off[b, i] + self.rep_len[b, i]].copy() for i in range(r)]
            st, got = oracle.rlc_decode_block(0, srcs, reps, self.seeds[b])
            self.status[b] = st
            self.rec[b] = mask([j in got for j in range(k)], k)
            self.n_recovered_blocks += st == DEC_RECOVERED
            for j, v in got.items():  # blk bytes: the source's own bytes, then zeros
                n = int(g.blk[b])
                assert len(v) == n and np.array_equal(v, g.src[b, j, :n]), (b, j)
                self.want[g.src_off[b, j]:g.src_off[b, j] + n] = v
            if zero_src and zero_src[0] == b and st == DEC_RECOVERED:
                assert zero_src[1] not in got
        self.zero_src, self.long_rep = zero_src, long_rep

    def tables(self, base):
        g = self.g
        rows_s = (base + g.src_off.reshape(-1)).astype(np.uint64)
        rows_r = (base + g.rep_off.reshape(-1)).astype(np.uint64)
        return (rows_s, g.src_len.reshape(-1).copy(), rows_r, self.rep_len.reshape(-1).copy(), g.blk.copy(),
                self.seeds.reshape(-1).copy(), self.sp.reshape(-1).copy(), self.rp.reshape(-1).copy())


def make_decode_case(rng, oracle, nb, k, r, L):
    return DecodeCase(rng, oracle, nb, k, r, L)


def _run_decode(eng, c, nb, k, r, L):
    pool = to_dev(c.pool_h)
    t = [to_dev(x) for x in c.tables(pool.data_ptr())]
    st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
    rec = torch.full((nb, 2), -1, dtype=torch.int64, device=DEV)
    eng.rlc_decode_rows_len(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], st, rec, nb, k, r, L)
    torch.cuda.synchronize()
    return pool.cpu().numpy(), st.cpu().numpy(), rec.cpu().numpy().view(np.uint64)


def _check_decode(c, got, st, rec, tag):
    assert np.array_equal(st, c.status), (tag, np.flatnonzero(st != c.status)[:8])
    assert np.array_equal(rec, c.rec), (tag, np.argwhere(rec != c.rec)[:8])
    # received rows, canaries, rows of unrecovered sources and of REF_UB blocks: untouched; recovered
    # rows: blk bytes, the source's own bytes then zeros
    assert np.array_equal(got, c.want), (tag, np.flatnonzero(got != c.want)[:8])


@pytest.mark.parametrize("k,r", SHAPES)
def test_decode_ragged_vs_oracle(eng, oracle, k, r):
    rng = np.random.default_rng(SEED + 1000 * k + r)
    blocks = recovered = 0
    for nb in NBLOCKS:
        c = make_decode_case(rng, oracle, nb, k, r, 1200)
        got, st, rec = _run_decode(eng, c, nb, k, r, 1200)
        _check_decode(c, got, st, rec, (k, r, nb))
        blocks += nb
        recovered += c.n_recovered_blocks
        if nb >= 3 and k >= 2 and c.status[2] == DEC_RECOVERED:
            assert c.zero_src[1] not in bits(rec[2], k)
    # vacuity guard: a run that mostly met REF_UB would check nothing
    assert recovered >= 0.9 * blocks, (recovered, blocks)


def test_decode_ragged_k64_r16_9000(eng, oracle):
    rng = np.random.default_rng(SEED + 9001)
    nb, k, r, L = 3, 64, 16, 9000
    c = make_decode_case(rng, oracle, nb, k, r, L)
    got, st, rec = _run_decode(eng, c, nb, k, r, L)
    _check_decode(c, got, st, rec, "k64 r16 L9000")


def _fixture_decode_cases(oracle):
    d = load("decode_cases.json")
    out = []
    for case in d["varlen_cases"] + d["cases"] + d["zero_cases"]:
        if case["scheme"] != "rlc" or case["k"] > 128 or case["r"] > 128:
            continue
        full = decode_sources(case)
        if max(len(s) for s in full) > 2052:
            continue  # the cases that fit a small pool
        out.append((case, full))
    return out


def test_decode_fixtures(eng, oracle):
    """Every RLC case of "varlen_cases", and the "cases" and "zero_cases" that fit, one block per call:
    status, recovered set, bytes and lengths as the reference recorded them."""
    import hashlib
    cases = _fixture_decode_cases(oracle)
    assert len(cases) > len([c for c in load("decode_cases.json")["varlen_cases"] if c["scheme"] == "rlc"]) > 0
    for case, full in cases:
        k, r, fbn = case["k"], case["r"], case["fbn"]
        reps_full = oracle.rlc_encode_block(fbn, full, r)[1]
        present = [j not in case["src_missing"] for j in range(k)]
        rpres = [i in case["rep_present"] for i in range(r)]
        if not any(rpres):
            continue  # no repair: no block length (the adapter completes such a block at submission)
        maxl = len(reps_full[[i for i in range(r) if rpres[i]][0]])
        L = max(pad4(max([maxl] + [len(s) for s in full])), 4)
        p = Pool(None)
        so = [p.add(max(maxl, len(full[j]))) for j in range(k)]
        ro = [p.add(len(reps_full[i])) for i in range(r)]
        pool_h = p.bytes()
        for j in range(k):
            if present[j]:
                pool_h[so[j]:so[j] + len(full[j])] = full[j]
        for i in range(r):
            if rpres[i]:
                pool_h[ro[i]:ro[i] + len(reps_full[i])] = reps_full[i]
        pool = to_dev(pool_h)
        base = pool.data_ptr()
        src_len = np.array([min(len(full[j]), maxl) if present[j] else 0 for j in range(k)], np.uint32)
        t = [to_dev(np.array([base + o for o in so], np.uint64)), to_dev(src_len),
             to_dev(np.array([base + o if rpres[i] else 0 for i, o in enumerate(ro)], np.uint64)),
             to_dev(np.array([len(reps_full[i]) if rpres[i] else 0 for i in range(r)], np.uint32)),
             to_dev(np.array([maxl], np.uint32)), to_dev(np.array([(fbn << 8) | i for i in range(r)], np.uint32)),
             to_dev(mask(present, k)), to_dev(mask(rpres, r))]
        st = torch.full((1,), 0xEE, dtype=torch.uint8, device=DEV)
        rec = torch.full((1, 2), -1, dtype=torch.int64, device=DEV)
        eng.rlc_decode_rows_len(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], st, rec, 1, k, r, L)
        torch.cuda.synchronize()
        got = pool.cpu().numpy()
        got_rec = bits(rec.cpu().numpy().view(np.uint64)[0], k) if int(st[0]) == DEC_RECOVERED else []
        tag = case["tag"]
        if case["crashed"]:  # the reference walks off its array here: flagged, nothing written
            assert got_rec == [] and np.array_equal(got, pool_h), tag
            continue
        assert {str(j) for j in got_rec} == set(case["recovered"]), tag
        want = pool_h.copy()
        for j in got_rec:
            row = got[so[j]:so[j] + maxl]
            assert hashlib.sha256(row.tobytes()).hexdigest() == case["recovered"][str(j)], (tag, j)
            assert case["recovered_len"][str(j)] == maxl, (tag, j)
            want[so[j]:so[j] + maxl] = row
        assert np.array_equal(got, want), tag  # nothing else written


# ---------------------------------------------------------------------------------- host forms
class HostMem:
    """Arrays in page-locked memory (fecgpu_host_alloc) or pageable numpy arrays."""

    def __init__(self, lib, pinned):
        self.lib, self.pinned, self.keep = lib, pinned, []
        lib.fecgpu_host_alloc.restype = C.c_void_p
        lib.fecgpu_host_alloc.argtypes = [C.c_size_t]
        lib.fecgpu_host_free.argtypes = [C.c_void_p]

    def array(self, a):
        a = np.ascontiguousarray(a)
        if not self.pinned:
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


@pytest.fixture(scope="module")
def hostpath(eng):
    from pquic_amd.engine import HostPath
    hp = HostPath(0, nstreams=2, chunk_bytes=1 << 20)  # small sub-batches: more than one per call
    yield hp
    hp.close()


def _dev_addr(lib, a):
    d = C.c_uint64(0)
    assert lib.fecgpu_host_device_address(a.ctypes.data, a.nbytes, C.byref(d)) == 0
    return d.value


@pytest.mark.parametrize("pinned", [False, True])
def test_host_forms(eng, oracle, hostpath, pinned):
    """The host forms on the same small batches: tables, lengths, masks, seeds, status and recovered in
    pageable arrays with the rows in device memory (everything copied), and all of it -- rows too -- in
    page-locked memory (everything in place).  A length violation is refused before anything is written."""
    lib = eng.lib
    rng = np.random.default_rng(SEED + 7 + pinned)
    hm = HostMem(lib, pinned)
    try:
        for nb, k, r in ((3, 4, 2), (65, 16, 4), (129, 2, 1)):
            L = 1200
            # encode
            g, fbn, pool_h, want = _encode_case(rng, oracle, nb, k, r, L)
            if pinned:
                pool = hm.array(pool_h)
                base = _dev_addr(lib, pool)
            else:
                pool = to_dev(pool_h)
                base = pool.data_ptr()
            rs, sl, rr, bl = [hm.array(x) for x in _encode_tables(g, base)]
            h_fbn = hm.array(fbn)
            bad = sl.copy() if not pinned else hm.array(sl)
            b_bad = nb - 1
            bad[b_bad * k] = bl[b_bad] + 1
            with pytest.raises(Exception, match="src_len above"):
                hostpath.rlc_encode_rows_len(rs, bad, rr, bl, nb, k, r, L, fbn=h_fbn)
            now = pool if pinned else pool.cpu().numpy()
            assert np.array_equal(now, pool_h), "a refused call wrote something"
            hostpath.rlc_encode_rows_len(rs, sl, rr, bl, nb, k, r, L, fbn=h_fbn)
            got = pool if pinned else pool.cpu().numpy()
            assert np.array_equal(got, want), ("encode", pinned, nb, k, r, np.flatnonzero(got != want)[:8])
            # decode
            c = make_decode_case(rng, oracle, nb, k, r, L)
            if pinned:
                pool = hm.array(c.pool_h)
                base = _dev_addr(lib, pool)
            else:
                pool = to_dev(c.pool_h)
                base = pool.data_ptr()
            t = [hm.array(x) for x in c.tables(base)]
            st = hm.array(np.full(nb, 0xEE, np.uint8))
            rec = hm.array(np.full((nb, 2), 0xFFFFFFFFFFFFFFFF, np.uint64))
            bad_bl = hm.array(t[4])
            bad_bl[0] = L + 4
            with pytest.raises(Exception, match="blk_len above"):
                hostpath.rlc_decode_rows_len(t[0], t[1], t[2], t[3], bad_bl, t[5], t[6], t[7], st, rec, nb, k, r, L)
            now = pool if pinned else pool.cpu().numpy()
            assert np.array_equal(now, c.pool_h) and (st == 0xEE).all(), "a refused call wrote something"
            hostpath.rlc_decode_rows_len(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], st, rec, nb, k, r, L)
            got = pool if pinned else pool.cpu().numpy()
            _check_decode(c, got, st, rec, ("host", pinned, nb, k, r))
    finally:
        hm.close()


def test_calls_are_counted(eng):
    nb, k, r, L = 70, 4, 2, 36
    src = torch.ones((nb, k, L), dtype=torch.uint8, device=DEV)
    rep = torch.zeros((nb, r, L), dtype=torch.uint8, device=DEV)
    rows_s = to_dev((src.data_ptr() + np.arange(nb * k, dtype=np.int64) * L).astype(np.uint64))
    rows_r = to_dev((rep.data_ptr() + np.arange(nb * r, dtype=np.int64) * L).astype(np.uint64))
    d_sl, d_bl = to_dev(np.full(nb * k, L, np.uint32)), to_dev(np.full(nb, L, np.uint32))
    s0 = eng.stats()
    eng.rlc_encode_rows_len(rows_s, d_sl, rows_r, d_bl, nb, k, r, L)
    d_rl = to_dev(np.full(nb * r, L, np.uint32))
    d_seed = to_dev(np.arange(nb * r, dtype=np.uint32))
    sp = to_dev(np.tile(np.array([0b1110, 0], np.uint64), nb))
    rp = to_dev(np.tile(np.array([0b11, 0], np.uint64), nb))
    st = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    rec = torch.zeros((nb, 2), dtype=torch.int64, device=DEV)
    eng.rlc_decode_rows_len(rows_s, d_sl, rows_r, d_rl, d_bl, d_seed, sp, rp, st, rec, nb, k, r, L)
    torch.cuda.synchronize()
    s1 = eng.stats()
    assert s1["encode_calls"] - s0["encode_calls"] == 1 and s1["encode_blocks"] - s0["encode_blocks"] == nb
    assert s1["decode_calls"] - s0["decode_calls"] == 1 and s1["decode_blocks"] - s0["decode_blocks"] == nb
