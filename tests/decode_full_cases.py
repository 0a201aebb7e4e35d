"""CPU side of the full-rank decode tests (test_decode_full_gpu.py): the erasure patterns, the
repairs, and the expected per-block verdicts from a GF(2^8) rank routine of its own -- nothing here
comes from the engine.  Ground truth for recovered bytes is the original sources."""
import functools

import numpy as np

from oracle_py import Oracle, synth_bytes

# (k, r, erasures, repairs present, blocks, seed)
TUPLES = [(16, 4, 4, 4, 4096, 11), (16, 6, 4, 6, 4096, 12), (32, 8, 8, 8, 2048, 13),
          (64, 16, 16, 16, 512, 14), (8, 8, 3, 5, 2048, 15), (100, 20, 20, 20, 256, 16)]

RECOVERED, NOTHING, REF_UB, SINGULAR = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def gf():
    return Oracle().gf_tables()  # mul[256][256], inv[256]


def gf_rank(M):
    """Rank over GF(2^8) of every matrix of M [nb][m][n] (uint8), by Gaussian elimination with a
    pivot search per column, all blocks at once."""
    mul, inv = gf()
    M = M.copy()
    nb, m, n = M.shape
    rank = np.zeros(nb, np.int64)
    rows = np.arange(m)[None, :]
    ar = np.arange(nb)
    for c in range(n):
        cand = (M[:, :, c] != 0) & (rows >= rank[:, None])
        has = cand.any(axis=1)
        if not has.any():
            continue
        bi = ar[has]
        piv = cand[has].argmax(axis=1)
        rk = rank[has]
        prow = M[bi, piv].copy()
        M[bi, piv] = M[bi, rk]
        prow = mul[inv[prow[:, c]][:, None], prow]  # pivot scaled to 1
        M[bi, rk] = prow
        f = M[bi, :, c].copy()
        f[rows[:, :] <= rk[:, None]] = 0            # only the rows below the pivot
        M[bi] ^= mul[f[:, :, None], prow[:, None, :]]
        rank[has] += 1
    return rank


def masks(nb, lists):
    m = np.zeros((nb, 2), np.uint64)
    for b, lst in enumerate(lists):
        for j in lst:
            m[b, int(j) >> 6] |= np.uint64(1) << np.uint64(int(j) & 63)
    return m


def bits(m, n):
    return [j for j in range(n) if (int(m[j >> 6]) >> (j & 63)) & 1]


class Case:
    """One batch: sources, repairs, masks and the CPU verdicts.
    full[b]   the received repairs' rows on the missing columns have rank e  (-> RECOVERED, else SINGULAR)
    first[b]  the first e received repairs alone already have rank e
    ref_st[b] reference mode's status, from the CPU restatement of the reference (liboracle)"""


def rows_for(seed_of, k, miss, present):
    """Coefficient rows [nb][p][e]: row of every received repair on the missing columns."""
    o = Oracle()
    nb = len(miss)
    out = np.zeros((nb, len(present[0]), len(miss[0])), np.uint8)
    for b in range(nb):
        for x, i in enumerate(present[b]):
            out[b, x] = o.coefs(seed_of(b, int(i)), k)[miss[b]]
    return out


def patterns(k, r, e, p, nb, seed):
    rng = np.random.default_rng(seed)
    miss, present = [], []
    for _ in range(nb):
        miss.append(np.array(sorted(rng.choice(k, e, replace=False))))
        present.append(np.array(sorted(rng.choice(r, p, replace=False))))
    return miss, present


@functools.lru_cache(maxsize=None)
def case(k, r, e, p, nb, seed, L, cut=None):
    """The batch of one tuple (fbn_base 0), cut to its first `cut` blocks if given."""
    o = Oracle()
    miss, present = patterns(k, r, e, p, nb, seed)
    if cut:
        nb, miss, present = cut, miss[:cut], present[:cut]
    c = Case()
    c.k, c.r, c.e, c.p, c.nb, c.L = k, r, e, p, nb, L
    c.miss, c.present = miss, present
    c.src = synth_bytes(nb * k * L, seed).reshape(nb, k, L)
    c.rep = o.rlc_encode_batch(c.src, r, 0)
    c.sp = masks(nb, [[j for j in range(k) if j not in set(m.tolist())] for m in miss])
    c.rp = masks(nb, present)
    rows = rows_for(lambda b, i: o.seed(b, i), k, miss, present)
    c.full = gf_rank(rows) == e
    c.first = gf_rank(rows[:, :e]) == e
    work = damaged(c)[0]
    c.ref_st, _ = o.rlc_decode_batch(work, c.rep, c.sp, c.rp, 0)
    return c


def damaged(c):
    """The buffers handed to the engine: missing sources filled with 0xA5, absent repairs with 0x5C."""
    work, rep = c.src.copy(), c.rep.copy()
    for b in range(c.nb):
        work[b, c.miss[b]] = 0xA5
        absent = np.setdiff1d(np.arange(c.r), c.present[b])
        rep[b, absent] = 0x5C
    return work, rep
