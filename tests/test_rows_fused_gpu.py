"""Ragged rows in one pass: fecgpu_rlc_encode_rows_fused / fecgpu_rlc_decode_rows_fused and their host forms
against the CPU oracle's per-block, per-length encode and decode, the reference's ragged fixtures, the
equal-length row forms and the staged *_rows_len forms.  Byte work: every comparison is exact and covers
the whole pool the rows live in (test_rows_len_gpu.Pool: canary bytes right behind every row, rows by
turns at offsets 0 / 4 / 8 / 12 mod 16), so a byte read past a source's length corrupts a result and a
byte written past a row fails the comparison.

The one freedom the fused decode has (fecgpu.h): a missing source of a RECOVERED block whose recovered
bit stays clear may have received blk_len bytes.  check_decode allows exactly those bytes to differ."""
import hashlib

import numpy as np
import pytest

import test_host_rows_gpu as HR
import test_rows_len_gpu as RL
from golden_io import load
from oracle_py import DEC_RECOVERED, Oracle
from test_rows_len_gpu import CANARY, DEV, Pool, Ragged, bits, mask, pad4, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20261020
SHAPES = [(1, 1), (2, 1), (4, 2), (4, 3), (16, 4), (32, 8), (16, 12), (64, 16), (8, 20)]
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


@pytest.fixture(scope="module")
def hostpath(eng):
    from pquic_amd.engine import HostPath
    hp = HostPath(0, nstreams=2, chunk_bytes=1 << 20)
    yield hp
    hp.close()


def diff(got, want):
    return np.flatnonzero(got != want)[:8]


# ---------------------------------------------------------------------------------- A. single block
def _single_cases():
    out = []
    for L in (16, 64):
        for n in sorted({min(x, L) for x in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64)}):
            out.append((L, n))
    return out


@pytest.mark.parametrize("L,n", _single_cases())
def test_a_single_block(eng, oracle, L, n):
    """k = 1, r = 1: one source of n bytes, the block as long as the source and one byte longer."""
    rng = np.random.default_rng([SEED, L, n])
    for blk in (n, n + 1):
        if blk > L:
            continue
        for turn in range(4):  # the source and the repair at each of the four offsets mod 16
            p = Pool(None)
            for _ in range(turn):
                p.add(4)
            so, ro = p.add(n), p.add(blk)
            pool_h = p.bytes()
            src = rng.integers(1, 256, n, dtype=np.uint8)
            pool_h[so:so + n] = src
            want = pool_h.copy()
            if n:
                ret, reps = oracle.rlc_encode_block(9, [src], 1)
                assert ret == 0 and len(reps[0]) == n
                want[ro:ro + n] = reps[0]
            want[ro + n:ro + blk] = 0  # past the longest source the repair is zero
            pool = to_dev(pool_h)
            base = pool.data_ptr()
            eng.rlc_encode_rows_fused(to_dev(np.array([base + so if n else 0], np.uint64)),
                                      to_dev(np.array([n], np.uint32)), to_dev(np.array([base + ro], np.uint64)),
                                      to_dev(np.array([blk], np.uint32)), 1, 1, 1, L, fbn_base=9)
            torch.cuda.synchronize()
            got = pool.cpu().numpy()
            assert np.array_equal(got, want), (L, n, blk, turn, diff(got, want) - ro)


# ---------------------------------------------------------------------------------- B. ragged encode
def _run_encode(eng, g, fbn, pool_h, nb, k, r, L):
    pool = to_dev(pool_h)
    t = [to_dev(x) for x in RL._encode_tables(g, pool.data_ptr())]
    eng.rlc_encode_rows_fused(t[0], t[1], t[2], t[3], nb, k, r, L, fbn=to_dev(fbn))
    torch.cuda.synchronize()
    return pool.cpu().numpy()


@pytest.mark.parametrize("k,r", SHAPES)
def test_b_encode_ragged_vs_oracle(eng, oracle, k, r):
    rng = np.random.default_rng([SEED, 1, k, r])
    for nb in NBLOCKS:
        g, fbn, pool_h, want = RL._encode_case(rng, oracle, nb, k, r, 1200)
        if nb >= 3:
            assert (g.blk[0], g.blk[1], g.blk[2]) == (0, 1, 1200) and (g.src_len == 0).any()
        got = _run_encode(eng, g, fbn, pool_h, nb, k, r, 1200)
        assert np.array_equal(got, want), (k, r, nb, diff(got, want))


class RaggedBlk(Ragged):
    """Ragged with the block lengths given (encode side)."""

    def __init__(self, rng, nb, k, r, L, blk):
        self.nb, self.k, self.r, self.L = nb, k, r, L
        self.blk = blk = np.asarray(blk, np.uint32)
        self.src_len = np.zeros((nb, k), np.uint32)
        self.src = np.zeros((nb, k, L), np.uint8)
        for b in range(nb):
            n = rng.integers(0, int(blk[b]) + 1, k)
            n[rng.integers(0, k)] = blk[b]
            self.src_len[b] = n
            for j in range(k):
                self.src[b, j, :n[j]] = rng.integers(1, 256, int(n[j]), dtype=np.uint8)
        self.pool = Pool(None)
        self.src_off = np.array([[self.pool.add(int(self.src_len[b, j])) for j in range(k)] for b in range(nb)],
                                np.int64).reshape(nb, k)
        self.rep_off = np.array([[self.pool.add(int(blk[b]) + 8) for _ in range(r)] for b in range(nb)],
                                np.int64).reshape(nb, r)


def _encode_want(oracle, g, fbn, pool_h):
    want = pool_h.copy()
    for b in range(g.nb):
        if g.blk[b] == 0:
            continue
        ret, reps = oracle.rlc_encode_block(int(fbn[b]), [g.src[b, j, :g.src_len[b, j]] for j in range(g.k)], g.r)
        assert ret == 0 and all(len(x) == g.blk[b] for x in reps)
        for i in range(g.r):
            want[g.rep_off[b, i]:g.rep_off[b, i] + g.blk[b]] = reps[i]
    return want


@pytest.mark.parametrize("k,r", [(4, 2), (16, 4)])
@pytest.mark.parametrize("L", [4, 8, 12, 36, 1208, 2052])
def test_b_encode_piece_and_chunk_geometry(eng, oracle, k, r, L):
    """The narrow piece widths (4, 8, 12), a last piece pulled back (36, 1208) and two column chunks (2052:
    chunks of 1040 bytes) with block lengths around the chunk boundary and of a few bytes, so that whole later
    chunks store nothing."""
    rng = np.random.default_rng([SEED, 2, k, r, L])
    for nb in (3, 65):
        if L == 2052:
            cb = 1040
            cand = list(range(cb - 3, cb + 4)) + [1, 2, 3, 4, 5]
            blk = [cand[(b * 5 + 3) % len(cand)] for b in range(nb)]
            g = RaggedBlk(rng, nb, k, r, L, blk)
            fbn = rng.integers(0, 1 << 24, nb).astype(np.uint32)
            pool_h = g.pool.bytes()
            g.fill_sources(pool_h)
            want = _encode_want(oracle, g, fbn, pool_h)
        else:
            g, fbn, pool_h, want = RL._encode_case(rng, oracle, nb, k, r, L)
        got = _run_encode(eng, g, fbn, pool_h, nb, k, r, L)
        assert np.array_equal(got, want), (k, r, L, nb, diff(got, want))


def test_b_encode_k64_r16_9000(eng, oracle):
    rng = np.random.default_rng([SEED, 3])
    nb, k, r, L = 3, 64, 16, 9000
    g, fbn, pool_h, want = RL._encode_case(rng, oracle, nb, k, r, L)
    got = _run_encode(eng, g, fbn, pool_h, nb, k, r, L)
    assert np.array_equal(got, want), diff(got, want)


# ---------------------------------------------------------------------------------- C. reference fixtures
def test_c_encode_varlen_fixtures(eng):
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
            eng.rlc_encode_rows_fused(d[0], d[1], d[2], d[3], 1, k, r, L, fbn_base=case["fbn"])
            torch.cuda.synchronize()
            got = pool.cpu().numpy()
            assert np.array_equal(got, want), (case.get("tag"), L, diff(got, want))


def test_c_decode_fixtures(eng, oracle):
    """Every variable-length RLC decode fixture (and the fixed-length and zero cases that fit a small pool),
    one block per call: status, recovered set, bytes and lengths as the reference recorded them."""
    cases = RL._fixture_decode_cases(oracle)
    nvar = len([c for c in load("decode_cases.json")["varlen_cases"] if c["scheme"] == "rlc"])
    assert len(cases) > nvar > 0
    for case, full in cases:
        k, r, fbn = case["k"], case["r"], case["fbn"]
        reps_full = oracle.rlc_encode_block(fbn, full, r)[1]
        present = [j not in case["src_missing"] for j in range(k)]
        rpres = [i in case["rep_present"] for i in range(r)]
        if not any(rpres):
            continue  # no repair: no block length
        maxl = len(reps_full[[i for i in range(r) if rpres[i]][0]])
        L0 = max(pad4(max([maxl] + [len(s) for s in full])), 4)
        for L in (L0, L0 + 52):
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
            eng.rlc_decode_rows_fused(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], st, rec, 1, k, r, L)
            torch.cuda.synchronize()
            got = pool.cpu().numpy()
            recovered_blk = int(st[0]) == DEC_RECOVERED
            got_rec = bits(rec.cpu().numpy().view(np.uint64)[0], k) if recovered_blk else []
            tag = (case["tag"], L)
            if case["crashed"]:  # the reference walks off its array here: flagged, nothing written
                assert got_rec == [] and np.array_equal(got, pool_h), tag
                continue
            assert {str(j) for j in got_rec} == set(case["recovered"]), tag
            want = pool_h.copy()
            for j in got_rec:
                row = got[so[j]:so[j] + maxl]
                assert hashlib.sha256(row.tobytes()).hexdigest() == case["recovered"][str(j)], (tag, j)
                assert case["recovered_len"][str(j)] == maxl, (tag, j)
            if recovered_blk:  # a missing source of a RECOVERED block may have received its maxl bytes
                for j in range(k):
                    if not present[j]:
                        want[so[j]:so[j] + maxl] = got[so[j]:so[j] + maxl]
            assert np.array_equal(got, want), tag  # nothing else written


# ---------------------------------------------------------------------------------- D. ragged decode
class FusedDecodeCase:
    """A ragged decode batch with random erasures of 1 .. min(k, r) sources and a random subset of the
    repairs (one block in eight receives one repair too few), per-repair seeds, one received source and one
    received repair longer than their block, and the oracle's verdict on it."""

    def __init__(self, rng, oracle, nb, k, r, L, longer=True, emin=1):
        g = self.g = Ragged(rng, nb, k, r, L, decode=True)
        self.nb, self.k, self.r, self.L = nb, k, r, L
        self.seeds = np.zeros((nb, r), np.uint32)
        for b in range(nb):
            for i in range(r):
                self.seeds[b, i] = ((int(rng.integers(0, 1 << 24)) << 8) | i) if b % 2 else int(rng.integers(0, 1 << 32))
        rep = RL.encode_seeded(oracle, g.src, self.seeds)
        self.rep_len = np.repeat(g.blk[:, None], r, 1).astype(np.uint32)
        self.src_len = g.src_len.copy()
        self.present = np.ones((nb, k), bool)
        self.rpresent = np.zeros((nb, r), bool)
        for b in range(nb):
            e = int(rng.integers(emin, min(k, r) + 1))
            self.present[b, rng.choice(k, e, replace=False)] = False
            nrep = e - 1 if b % 8 == 7 else int(rng.integers(e, r + 1))
            self.rpresent[b, rng.choice(r, nrep, replace=False)] = True
        pool_h = g.pool.bytes()
        g.fill_sources(pool_h, self.present)
        for b in range(nb):
            for i in np.flatnonzero(self.rpresent[b]):
                n = int(g.blk[b])
                pool_h[g.rep_off[b, i]:g.rep_off[b, i] + n] = rep[b, i, :n]
        if longer:
            b = nb - 1
            got_reps = np.flatnonzero(self.rpresent[b])
            if len(got_reps) >= 2:  # not the first one present: the reference takes the block's length from that
                i = int(got_reps[-1])
                self.rep_len[b, i] += 8
                o = g.rep_off[b, i] + int(g.blk[b])
                pool_h[o:o + 8] = rng.integers(1, 256, 8, dtype=np.uint8)
            # a received source said to be longer than its block: the canaries behind it must not be read
            j = int(np.flatnonzero(self.present[b])[0]) if self.present[b].any() else None
            if j is not None and g.src_len[b, j] == g.blk[b]:
                self.src_len[b, j] += 8
        self.pool_h = pool_h
        self.status = np.zeros(nb, np.uint8)
        self.rec = np.zeros((nb, 2), np.uint64)
        self.sp = np.stack([mask(self.present[b], k) for b in range(nb)])
        self.rp = np.stack([mask(self.rpresent[b], r) for b in range(nb)])
        self.rows = {}  # (b, j) -> the bytes a set bit promises
        for b in range(nb):
            srcs = [g.src[b, j, :g.src_len[b, j]] if self.present[b, j] else None for j in range(k)]
            reps = [pool_h[g.rep_off[b, i]:g.rep_off[b, i] + self.rep_len[b, i]].copy() if self.rpresent[b, i] else None
                    for i in range(r)]
            st, got = oracle.rlc_decode_block(0, srcs, reps, self.seeds[b])
            self.status[b] = st
            self.rec[b] = mask([j in got for j in range(k)], k)
            for j, v in got.items():
                n = int(g.blk[b])
                assert len(v) == n and np.array_equal(v, g.src[b, j, :n]), (b, j)
                self.rows[(b, j)] = v
        self.n_recovered = int((self.status == DEC_RECOVERED).sum())

    def tables(self, base):
        g = self.g
        rows_s = (base + g.src_off.reshape(-1)).astype(np.uint64)
        rows_r = (base + g.rep_off.reshape(-1)).astype(np.uint64)
        rows_r[~self.rpresent.reshape(-1)] = 0  # an absent repair is never looked at
        return (rows_s, self.src_len.reshape(-1).copy(), rows_r, self.rep_len.reshape(-1).copy(), g.blk.copy(),
                self.seeds.reshape(-1).copy(), self.sp.reshape(-1).copy(), self.rp.reshape(-1).copy())


def check_decode(c, got, st, rec, tag):
    """Status and recovered words are the oracle's; every row whose bit is set holds the source; a missing
    source of a RECOVERED block whose bit is clear may hold anything in its blk bytes; every other byte of
    the pool -- received rows, rows of blocks that are not RECOVERED, canaries -- is untouched."""
    g = c.g
    assert np.array_equal(st, c.status), (tag, np.flatnonzero(st != c.status)[:8])
    assert np.array_equal(rec, c.rec), (tag, np.argwhere(rec != c.rec)[:8])
    want = c.pool_h.copy()
    for (b, j), v in c.rows.items():
        want[g.src_off[b, j]:g.src_off[b, j] + len(v)] = v
    for b in np.flatnonzero(c.status == DEC_RECOVERED):
        for j in np.flatnonzero(~c.present[b]):
            if (b, j) not in c.rows:
                o, n = g.src_off[b, j], int(g.blk[b])
                want[o:o + n] = got[o:o + n]
    assert np.array_equal(got, want), (tag, diff(got, want))


def run_decode(eng, c, fused=True):
    nb, k, r, L = c.nb, c.k, c.r, c.L
    pool = to_dev(c.pool_h)
    t = [to_dev(x) for x in c.tables(pool.data_ptr())]
    st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
    rec = torch.full((nb, 2), -1, dtype=torch.int64, device=DEV)
    call = eng.rlc_decode_rows_fused if fused else eng.rlc_decode_rows_len
    call(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], st, rec, nb, k, r, L)
    torch.cuda.synchronize()
    return pool.cpu().numpy(), st.cpu().numpy(), rec.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("k,r", SHAPES)
def test_d_decode_ragged_vs_oracle(eng, oracle, k, r):
    rng = np.random.default_rng([SEED, 4, k, r])
    for nb in NBLOCKS:
        c = FusedDecodeCase(rng, oracle, nb, k, r, 1200)
        if nb >= 65:  # before the device runs: most blocks are recovered, and not all of them
            assert 4 * c.n_recovered >= 3 * nb and c.n_recovered < nb, (k, r, nb, c.n_recovered)
        got, st, rec = run_decode(eng, c)
        check_decode(c, got, st, rec, (k, r, nb))


def test_d_decode_more_than_16_unknowns(eng, oracle):
    """k = 32, r = 20 with 17 .. 20 sources missing: two data passes and k_rlc_finalize."""
    rng = np.random.default_rng([SEED, 5])
    nb, k, r, L = 9, 32, 20, 1200
    c = FusedDecodeCase(rng, oracle, nb, k, r, L, emin=17)
    assert ((~c.present).sum(1) > 16).all() and c.n_recovered >= 6
    got, st, rec = run_decode(eng, c)
    check_decode(c, got, st, rec, "e > 16")


def test_d_decode_k64_r16_9000(eng, oracle):
    rng = np.random.default_rng([SEED, 6])
    c = FusedDecodeCase(rng, oracle, 3, 64, 16, 9000)
    got, st, rec = run_decode(eng, c)
    check_decode(c, got, st, rec, "k64 r16 L9000")


# ---------------------------------------------------------------------------------- E. equal lengths
E_SHAPES = [(16, 4, 1200, 129), (4, 2, 36, 65), (64, 16, 1200, 3)]


@pytest.mark.parametrize("k,r,L,nb", E_SHAPES)
def test_e_equal_lengths_match_the_row_forms(eng, k, r, L, nb):
    """Every length equal to symbol_size: the pool is byte-identical to fecgpu_rlc_encode_rows /
    fecgpu_rlc_decode_rows (rows L + 4 apart, canaries between)."""
    rng = np.random.default_rng([SEED, 7, k])
    st_ = L + 4
    image = np.full(nb * (k + r) * st_ + 64, CANARY, np.uint8)
    rows = image[:nb * (k + r) * st_].reshape(nb * (k + r), st_)
    rows[:nb * k, :L] = rng.integers(0, 256, (nb * k, L), dtype=np.uint8)
    pools = [to_dev(image), to_dev(image)]
    tab = lambda p, first, n: to_dev((p.data_ptr() + (first + np.arange(n, dtype=np.int64)) * st_).astype(np.uint64))  # noqa: E731
    rs, rr = [tab(p, 0, nb * k) for p in pools], [tab(p, nb * k, nb * r) for p in pools]
    d_sl, d_rl, d_bl = (to_dev(np.full(n, L, np.uint32)) for n in (nb * k, nb * r, nb))
    eng.rlc_encode_rows(rs[0], rr[0], nb, k, r, L, fbn_base=77)
    eng.rlc_encode_rows_fused(rs[1], d_sl, rr[1], d_bl, nb, k, r, L, fbn_base=77)
    torch.cuda.synchronize()
    a, b = pools[0].cpu().numpy(), pools[1].cpu().numpy()
    assert np.array_equal(a, b), diff(a, b)
    assert (a[:nb * (k + r) * st_].reshape(-1, st_)[nb * k:, :L] != CANARY).any()
    # decode: erase 1 .. min(k, r) sources per block (garbage in their rows), seeds (fbn << 8) | i
    sp = np.zeros((nb, 2), np.uint64)
    garbage = a.copy()
    g_rows = garbage[:nb * (k + r) * st_].reshape(nb * (k + r), st_)
    for blk in range(nb):
        present = np.ones(k, bool)
        present[rng.choice(k, 1 + blk % min(k, r), replace=False)] = False
        sp[blk] = mask(present, k)
        g_rows[blk * k + np.flatnonzero(~present), :L] = 0xA5
    rp = np.tile(mask([True] * r, r), (nb, 1))
    seeds = (((77 + np.arange(nb, dtype=np.uint64)) << 8)[:, None] | np.arange(r, dtype=np.uint64)[None, :]).astype(np.uint32)
    pools = [to_dev(garbage), to_dev(garbage)]
    rs, rr = [tab(p, 0, nb * k) for p in pools], [tab(p, nb * k, nb * r) for p in pools]
    outs = []
    for i, p in enumerate(pools):
        st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
        rec = torch.full((nb, 2), -1, dtype=torch.int64, device=DEV)
        args = (to_dev(seeds.reshape(-1)), to_dev(sp.reshape(-1)), to_dev(rp.reshape(-1)), st, rec)
        if i == 0:
            ws = eng.alloc_workspace(nb, k, r)
            rc = eng.lib.fecgpu_rlc_decode_rows(rs[0].data_ptr(), rr[0].data_ptr(), nb, k, r, L, *[x.data_ptr() for x in args],
                                                ws.data_ptr(), ws.numel(), eng._stream(None))
            assert rc == 0, eng.err()
        else:
            eng.rlc_decode_rows_fused(rs[1], d_sl, rr[1], d_rl, d_bl, *args, nb, k, r, L)
        torch.cuda.synchronize()
        outs.append((p.cpu().numpy(), st.cpu().numpy(), rec.cpu().numpy()))
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    ok = outs[0][1] == DEC_RECOVERED  # a singular draw is possible, but rare
    assert 4 * ok.sum() >= 3 * nb
    assert np.array_equal(outs[0][0], outs[1][0]), diff(outs[0][0], outs[1][0])
    src_rows = lambda x: x[:nb * k * st_].reshape(nb, k, st_)[ok]  # noqa: E731
    assert np.array_equal(src_rows(outs[1][0]), src_rows(a)), "recovered blocks hold the sources again"


@pytest.mark.parametrize("k,r,L,nb", E_SHAPES)
def test_e_ragged_matches_rows_len(eng, oracle, k, r, L, nb):
    """Ragged input: recovered[], status[] and every row whose bit is set are those of the staged form."""
    rng = np.random.default_rng([SEED, 8, k])
    g, fbn, pool_h, _ = RL._encode_case(rng, oracle, nb, k, r, L)
    outs = []
    for call in (eng.rlc_encode_rows_len, eng.rlc_encode_rows_fused):
        pool = to_dev(pool_h)
        t = [to_dev(x) for x in RL._encode_tables(g, pool.data_ptr())]
        call(t[0], t[1], t[2], t[3], nb, k, r, L, fbn=to_dev(fbn))
        torch.cuda.synchronize()
        outs.append(pool.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), diff(outs[0], outs[1])
    c = FusedDecodeCase(rng, oracle, nb, k, r, L, longer=False)
    staged, fused = run_decode(eng, c, fused=False), run_decode(eng, c, fused=True)
    assert np.array_equal(staged[1], fused[1]) and np.array_equal(staged[2], fused[2])
    for (b, j), v in c.rows.items():
        o = c.g.src_off[b, j]
        assert np.array_equal(staged[0][o:o + len(v)], fused[0][o:o + len(v)]), (b, j)
    check_decode(c, fused[0], fused[1], fused[2], "ragged against rows_len")


# ---------------------------------------------------------------------------------- F. host forms
class EncodeRowsFused(HR.EncodeRowsLen):
    def host(self, lib, ctx, a):
        p = HR._p
        return lib.fecgpu_rlc_encode_rows_fused_host(ctx, p(a["src_rows"]), p(a["src_len"]), p(a["rep_rows"]),
                                                     p(a["blk_len"]), *self.d, p(a["fbn"]))

    def device(self, eng, a):
        eng.rlc_encode_rows_fused(a["src_rows"], a["src_len"], a["rep_rows"], a["blk_len"], *self.d, fbn_base=0,
                                  fbn=a["fbn"])


class DecodeRowsFused(HR.DecodeRowsLen):
    def __init__(self, *a):
        super().__init__(*a)
        self.want = None  # an unrecovered row of a RECOVERED block may be written: held to the device form instead

    def host(self, lib, ctx, a):
        p = HR._p
        return lib.fecgpu_rlc_decode_rows_fused_host(ctx, p(a["src_rows"]), p(a["src_len"]), p(a["rep_rows"]),
                                                     p(a["rep_len"]), p(a["blk_len"]), *self.d, p(a["seeds"]),
                                                     p(a["sp"]), p(a["rp"]), p(a["status"]), p(a["recovered"]))

    def device(self, eng, a):
        r = self.d[2]  # with r == 0 the source tables stand in for the repair tables
        eng.rlc_decode_rows_fused(a["src_rows"], a["src_len"], a["rep_rows"] if r else a["src_rows"],
                                  a["rep_len"], a["blk_len"], a["seeds"], a["sp"], a["rp"], a["status"],
                                  a["recovered"], *self.d)


FUSED = {"encode": EncodeRowsFused, "decode": DecodeRowsFused}


def make_fused_form(name, eng, oracle, nb, k, r, L, **kw):
    rng = np.random.default_rng([SEED, 9, name == "decode", nb, k, r, L])
    return FUSED[name](rng, eng, oracle, nb, k, r, L, **kw)


@pytest.mark.parametrize("name", ["encode", "decode"])
def test_f_host_tables_page_locked_pageable_and_mixed(eng, oracle, hostpath, name):
    """65 blocks of k16 r4 L1200 (two sub-batches at 1 MiB), rows page-locked: every table page-locked, all
    pageable, and one pageable table among page-locked ones leave the device form's bytes, status and masks."""
    form = make_fused_form(name, eng, oracle, 65, 16, 4, 1200)
    ref = HR.run_device(eng, form)
    if name == "encode":
        assert np.array_equal(ref.pool, form.want)
    pinned = HR.run_host(eng, hostpath, form, True)
    pageable = HR.run_host(eng, hostpath, form, False)
    mixed = HR.run_host(eng, hostpath, form, True, pageable=(form.order[-1],))
    for got, tag in ((pinned, "page-locked"), (pageable, "pageable"), (mixed, "mixed")):
        HR.assert_same(got, ref, tag)
        if got.status is not None:
            assert 0xEE not in got.status
    assert (mixed.hits, mixed.misses) == (len(form.order) - 1, 1), (mixed.hits, mixed.misses)


@pytest.mark.parametrize("name", ["encode", "decode"])
def test_f_host_sliced_equals_the_device_form(eng, oracle, hostpath, name):
    """100 blocks of k4 r2 L1200 cut into slices of 32 blocks while the hooks count as in use."""
    form = make_fused_form(name, eng, oracle, 100, 4, 2, 1200)
    old = {n: eng.get_knob(n) for n in ("yield_always", "yield_slice_kb")}
    try:
        eng.set_knob("yield_always", 1)
        eng.set_knob("yield_slice_kb", 1)
        cut = HR.run_host(eng, hostpath, form, True)
    finally:
        for n, v in old.items():
            eng.set_knob(n, v)
    assert cut.slices >= 4, cut.slices
    HR.assert_same(cut, HR.run_device(eng, form), "sliced against the device form")


@pytest.mark.parametrize("tables_pinned", [False, True])
def test_f_host_decode_without_repairs(eng, oracle, hostpath, tables_pinned):
    nb, k = 33, 4
    form = make_fused_form("decode", eng, oracle, nb, k, 0, 36)
    a = form.arrays(0)
    assert a["rep_rows"] is None and a["seeds"] is None and a["rep_len"] is None
    got = HR.run_host(eng, hostpath, form, tables_pinned)
    HR.assert_same(got, HR.run_device(eng, form), "r == 0")
    assert 0xEE not in got.status
    assert np.array_equal(got.pool, form.image), "a decode without repairs wrote a row"


# ---------------------------------------------------------------------------------- G. counters
def test_g_calls_are_counted(eng):
    nb, k, r, L = 70, 4, 2, 36
    src = torch.ones((nb, k, L), dtype=torch.uint8, device=DEV)
    rep = torch.zeros((nb, r, L), dtype=torch.uint8, device=DEV)
    rows_s = to_dev((src.data_ptr() + np.arange(nb * k, dtype=np.int64) * L).astype(np.uint64))
    rows_r = to_dev((rep.data_ptr() + np.arange(nb * r, dtype=np.int64) * L).astype(np.uint64))
    d_sl, d_bl = to_dev(np.full(nb * k, L, np.uint32)), to_dev(np.full(nb, L, np.uint32))
    s0 = eng.stats()
    eng.rlc_encode_rows_fused(rows_s, d_sl, rows_r, d_bl, nb, k, r, L)
    d_rl = to_dev(np.full(nb * r, L, np.uint32))
    d_seed = to_dev(np.arange(nb * r, dtype=np.uint32))
    sp = to_dev(np.tile(np.array([0b1110, 0], np.uint64), nb))
    rp = to_dev(np.tile(np.array([0b11, 0], np.uint64), nb))
    st = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    rec = torch.zeros((nb, 2), dtype=torch.int64, device=DEV)
    eng.rlc_decode_rows_fused(rows_s, d_sl, rows_r, d_rl, d_bl, d_seed, sp, rp, st, rec, nb, k, r, L)
    torch.cuda.synchronize()
    s1 = eng.stats()
    assert s1["encode_calls"] - s0["encode_calls"] == 1 and s1["encode_blocks"] - s0["encode_blocks"] == nb
    assert s1["decode_calls"] - s0["decode_calls"] == 1 and s1["decode_blocks"] - s0["decode_blocks"] == nb
