"""Span decode: an independent numpy model of fecgpu_rlc_span_decode's semantics (include/fecgpu.h).

Built from the oracle's TinyMT32 coefficients (Oracle.coefs) and GF(2^8) tables (Oracle.gf_tables) alone;
it shares no code with the engine.  A batch of spans of one width K and R repair slots is solved at once:
the m x n matrix of the present, valid repairs on the missing columns is brought to reduced row echelon
form by offering the rows in ascending slot order (a row that reduces to zero is dependent, or zero on
every missing column, and is not selected), and a missing column is determined iff the row with its
pivot is zero on every other missing column."""
from __future__ import annotations

import numpy as np

RECOVERED, NOTHING, REF_UB, SINGULAR = 0, 1, 2, 3


def bits(mask, n):
    """(nb, 2) u64 presence masks -> (nb, n) bool"""
    m = np.ascontiguousarray(mask).view(np.uint64).reshape(-1, 2)
    j = np.arange(n)
    return ((m[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def pack(b):
    """(nb, n) bool -> (nb, 2) u64"""
    out = np.zeros((b.shape[0], 2), np.uint64)
    for j in range(b.shape[1]):
        out[:, j >> 6] |= b[:, j].astype(np.uint64) << np.uint64(j & 63)
    return out


class Solution:
    """What the model says of a batch: valid / selected (nb, R), miss / det (nb, K), status (nb,), the
    coefficient rows C (nb, R, K) and, when asked for, T (nb, K, R): T[b, u] combines the repairs'
    syndromes into determined source u."""


class SpanModel:
    def __init__(self, oracle=None):
        from oracle_py import Oracle
        self.o = oracle or Oracle()
        self.mul, self.inv = self.o.gf_tables()
        self._coefs = {}

    def coef_row(self, seed, nss):
        key = (int(seed), int(nss))
        if key not in self._coefs:
            self._coefs[key] = self.o.coefs(key[0], key[1]).copy()
        return self._coefs[key]

    def matrix(self, K, seed, off, nss, valid):
        """Coefficient rows (nb, R, K): zero outside [off, off + nss), coefs(seed, nss) inside."""
        nb, R = seed.shape
        C = np.zeros((nb, R, K), np.uint8)
        if not valid.any():
            return C
        keys = np.stack([seed.astype(np.int64), off.astype(np.int64), nss.astype(np.int64)], -1)[valid]
        uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
        rows = np.zeros((len(uniq), K), np.uint8)
        for x, (s, o, w) in enumerate(uniq):
            rows[x, o:o + w] = self.coef_row(s, w)
        C[valid] = rows[inverse.reshape(-1)]
        return C

    def _eliminate(self, A, miss, with_T):
        """Greedy reduced row echelon form of A (nb, R, K) on the columns `miss`, rows offered in ascending
        order.  Returns pivot (nb, R): the pivot column of an accepted row, else -1; lone (nb, R): the
        accepted row is zero on every other missing column; T (nb, R, R) or None: row e as a combination of
        the original rows."""
        nb, R, K = A.shape
        order = np.argsort(~miss, axis=1, kind="stable")  # missing columns first, ascending
        nmax = max(int(miss.sum(1).max()) if nb else 0, 1)
        order = order[:, :nmax]
        W = np.take_along_axis(A, order[:, None, :], axis=2) * np.take_along_axis(miss, order, 1)[:, None, :]
        W = W.astype(np.uint8)
        # rows that are zero on the missing columns can never be accepted: the others first, in ascending order
        live = (W != 0).any(2)
        rmax = max(int(live.sum(1).max()) if nb else 0, 1)
        rows = np.argsort(~live, axis=1, kind="stable")[:, :rmax]
        W = np.take_along_axis(W, rows[:, :, None], axis=1)
        if with_T:
            W = np.concatenate([W, np.eye(R, dtype=np.uint8)[rows]], axis=2)
        pivot = np.full((nb, rmax), -1, np.int64)
        for e in range(rmax):
            nz = W[:, e, :nmax] != 0
            idx = np.nonzero(nz.any(1))[0]
            if idx.size == 0:
                continue
            pe = nz[idx].argmax(1)  # the first missing column where the reduced row is non-zero
            rowe = self.mul[self.inv[W[idx, e, pe]][:, None], W[idx, e, :]]
            W[idx, e, :] = rowe
            f = W[idx, :, pe].copy()  # (ni, R): every other row's entry in the pivot column
            f[:, e] = 0
            W[idx] ^= self.mul[f[:, :, None], rowe[:, None, :]]
            pivot[idx, e] = order[idx, pe]
        lone = (pivot >= 0) & ((W[:, :, :nmax] != 0).sum(2) == 1)
        # back to the slots' own numbering
        pivot_r = np.full((nb, R), -1, np.int64)
        lone_r = np.zeros((nb, R), bool)
        np.put_along_axis(pivot_r, rows, pivot, axis=1)
        np.put_along_axis(lone_r, rows, lone, axis=1)
        T = None
        if with_T:
            T = np.zeros((nb, R, R), np.uint8)
            np.put_along_axis(T, rows[:, :, None], W[:, :, nmax:], axis=1)
        return pivot_r, lone_r, T

    def solve(self, K, seed, off, nss, sp, rp, with_T=False):
        seed = np.asarray(seed, np.uint32)
        off = np.asarray(off, np.uint8)
        nss = np.asarray(nss, np.uint8)
        nb, R = seed.shape
        s = Solution()
        s.K, s.R = K, R
        s.valid = bits(rp, R) & (nss >= 1) & (off.astype(np.int64) + nss.astype(np.int64) <= K)
        s.miss = ~bits(sp, K)
        s.C = self.matrix(K, seed, off, nss, s.valid)
        pivot, lone, T = self._eliminate(s.C, s.miss, with_T)
        s.selected = pivot >= 0
        s.det = np.zeros((nb, K), bool)
        b, e = np.nonzero(lone)
        s.det[b, pivot[b, e]] = True
        s.T = None
        if with_T:
            s.T = np.zeros((nb, K, R), np.uint8)
            s.T[b, pivot[b, e]] = T[b, e]
        n, m = s.miss.sum(1), s.valid.sum(1)
        s.status = np.where((n == 0) | (m == 0), NOTHING, np.where(s.det.any(1), RECOVERED, SINGULAR)).astype(np.uint8)
        return s

    def recovered(self, s, original):
        """recovered[]: the determined sources whose bytes are not all zero"""
        return pack(s.det & (original != 0).any(2))

    def expected_rows(self, s, work, original):
        """The rows after the decode: determined rows hold the original symbol, every other row what it held."""
        return np.where(s.det[:, :, None], original, work)

    def solve_bytes(self, s, src, rep):
        """The determined sources computed from the received symbols alone (s from solve(with_T=True)):
        x_u = sum_i T[u][i] * (rep_i - sum_{present j} C[i][j] * src_j).  Returns a copy of src with them."""
        out = src.copy()
        for b in np.nonzero(s.det.any(1))[0]:
            syn = {}
            for i in np.nonzero(s.selected[b])[0]:
                v = rep[b, i].copy()
                for j in np.nonzero(~s.miss[b] & (s.C[b, i] != 0))[0]:
                    v ^= self.mul[s.C[b, i, j]][src[b, j]]
                syn[i] = v
            for u in np.nonzero(s.det[b])[0]:
                x = np.zeros(src.shape[2], np.uint8)
                for i, v in syn.items():
                    if s.T[b, u, i]:
                        x ^= self.mul[s.T[b, u, i]][v]
                out[b, u] = x
        return out

    def encode(self, s, src):
        """The repairs of the model's coefficient rows on full rows src (nb, K, L) -> (nb, R, L)"""
        nb, R, K = s.C.shape
        rep = np.zeros((nb, R, src.shape[2]), np.uint8)
        for b in range(nb):
            for i in range(R):
                for j in np.nonzero(s.C[b, i])[0]:
                    rep[b, i] ^= self.mul[s.C[b, i, j]][src[b, j]]
        return rep

    def windows_alone(self, s, off, nss, propagate=False):
        """What decoding each window by itself in full-rank mode determines (nb, K) bool: window (off, nss)
        with the repairs sent for it recovers all its missing sources iff it has at least as many repairs
        as losses and their matrix on the losses has full column rank, else none.  propagate: a recovered
        source counts as received by the windows decoded after it, until nothing more is recovered."""
        off = np.asarray(off, np.int64)
        nss = np.asarray(nss, np.int64)
        nb, R = off.shape
        miss = s.miss.copy()
        wins = np.unique(np.stack([off, nss], -1)[s.valid], axis=0) if s.valid.any() else []
        changed = True
        while changed:
            changed = False
            start = miss if propagate else s.miss
            for o, w in wins:
                rows = s.valid & (off == o) & (nss == w)
                mw = np.zeros_like(miss)
                mw[:, o:o + w] = start[:, o:o + w]
                n, m = mw.sum(1), rows.sum(1)
                todo = np.nonzero((n > 0) & (m >= n))[0]
                if todo.size == 0:
                    continue
                pivot, _, _ = self._eliminate(s.C[todo] * rows[todo][:, :, None], mw[todo], False)
                full = todo[(pivot >= 0).sum(1) == n[todo]]
                if full.size and (miss[full] & mw[full]).any():
                    miss[full] &= ~mw[full]
                    changed = propagate
        return s.miss & ~miss
