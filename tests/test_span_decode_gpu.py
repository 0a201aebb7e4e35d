"""Span decode (fecgpu_rlc_span_decode and its row forms) on the device.  Streams are encoded with the
engine's own rlc_window_encode; the originals are kept, missing rows and the rows of repairs that must not be
used are poisoned.  Every case compares status, recovered[] and every row with the numpy model
(span_model.py) and the originals, byte for byte: determined rows hold the original symbol, every other row
what it held before."""
import numpy as np
import pytest

from oracle_py import synth_bytes
from span_model import NOTHING, RECOVERED, SINGULAR, SpanModel, bits, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
MISSING, UNUSED, SENTINEL = 0xA5, 0x5A, 0xC3


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(0)


@pytest.fixture(scope="module")
def model():
    return SpanModel()


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


class Spans:
    """nb spans of K columns with one layout of windows: windows = [(off, nss, r), ...], r repairs each
    (seeds 0..r-1: window blocks carry block number 0), R slots in that order."""

    def __init__(self, K, L, nb, windows, data_seed=1):
        self.K, self.L, self.nb, self.windows = K, L, nb, windows
        self.R = sum(w[2] for w in windows)
        self.seed = np.tile(np.concatenate([np.arange(r) for _, _, r in windows]).astype(np.uint32), (nb, 1))
        self.off = np.tile(np.concatenate([np.full(r, o) for o, _, r in windows]).astype(np.uint8), (nb, 1))
        self.nss = np.tile(np.concatenate([np.full(r, n) for _, n, r in windows]).astype(np.uint8), (nb, 1))
        self.src = synth_bytes(nb * K * L, data_seed).reshape(nb, K, L).copy()
        for b in range(3, nb, 7):  # all-zero symbols: written when determined, their recovered bit clear
            self.src[b, b % K] = 0
        self.rep = None

    def encode(self, eng):
        """Window (off, nss, r) of every span in one rlc_window_encode call: the spans' columns are one
        stream, the windows of consecutive spans K symbols apart."""
        if self.rep is None:
            stream = to_dev(self.src.reshape(self.nb * self.K, self.L))
            parts = []
            for o, n, r in self.windows:
                out = torch.empty((self.nb, r, self.L), dtype=torch.uint8, device=DEV)
                eng.rlc_window_encode(stream[o:], out, self.nb, self.K, n, r, self.L)
                parts.append(out)
            torch.cuda.synchronize()
            self.rep = torch.cat(parts, dim=1).cpu().numpy()
        return self.rep


def new_out(nb):
    return (torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV),
            torch.full((nb, 2), -1, dtype=torch.int64, device=DEV))


def host_out(out):
    return out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint64)


def coverage(s):
    """(fully, partially, not) determined spans among those with losses and repairs"""
    live = s.status != NOTHING
    full = live & (s.det == s.miss).all(1)
    part = live & s.det.any(1) & ~full
    none = live & ~s.det.any(1)
    return full, part, none


def damaged(fx, rep, s):
    """Missing sources poisoned; so is every repair the decode must not read (absent, invalid, unselected)."""
    work = np.where(s.miss[:, :, None], np.uint8(MISSING), fx.src)
    rep_w = np.where(s.selected[:, :, None], rep, np.uint8(UNUSED))
    return work, rep_w


def check(model, fx, s, work, got, st, rec):
    assert np.array_equal(st, s.status), np.nonzero(st != s.status)[0][:10]
    exp_rec = model.recovered(s, fx.src)
    assert np.array_equal(rec, exp_rec), np.nonzero((rec != exp_rec).any(1))[0][:10]
    want = model.expected_rows(s, work, fx.src)
    bad = np.nonzero((got != want).any(axis=2))
    assert bad[0].size == 0, list(zip(*bad))[:10]


def run_packed(eng, model, fx, present, rpresent, off=None, nss=None, sel=None):
    """One fecgpu_rlc_span_decode call on the spans `sel` of fx, checked against the model."""
    off = fx.off if off is None else off
    nss = fx.nss if nss is None else nss
    sp, rp = pack(present), pack(rpresent)
    s = model.solve(fx.K, fx.seed, off, nss, sp, rp)
    work, rep_w = damaged(fx, fx.encode(eng), s)
    idx = np.arange(fx.nb) if sel is None else np.asarray(sel)
    w, r = to_dev(work[idx]), to_dev(rep_w[idx])
    out = new_out(idx.size)
    eng.rlc_span_decode(w, r, to_dev(fx.seed[idx]), to_dev(off[idx]), to_dev(nss[idx]), to_dev(sp[idx]),
                        to_dev(rp[idx]), *out, fx.K, fx.R, fx.L, nspans=idx.size)
    torch.cuda.synchronize()
    st, rec = host_out(out)
    got = w.cpu().numpy()
    assert np.array_equal(r.cpu().numpy(), rep_w[idx])  # no repair row is written
    sub = sub_solution(s, idx)
    sub_fx = type("Sub", (), dict(src=fx.src[idx]))
    check(model, sub_fx, sub, work[idx], got, st, rec)
    return s, work, rep_w, got, st, rec


def sub_solution(s, idx):
    t = type(s)()
    for name in ("valid", "miss", "selected", "det", "status", "C"):
        setattr(t, name, getattr(s, name)[idx])
    return t


def random_losses(fx, seed, p_src, p_rep):
    rng = np.random.default_rng(seed)
    return rng.random((fx.nb, fx.K)) >= p_src, rng.random((fx.nb, fx.R)) >= p_rep


# --------------------------------------------------------------------------------- 1. the point of the feature
def test_two_losses_in_one_window_need_the_neighbouring_windows(eng, model):
    """k30 r1 step 5, spans of 55 columns (six windows), two losses in the five columns every window covers:
    no window has two repairs, so fecgpu_rlc_decode_full window by window recovers neither; the span decode
    recovers both from the six repairs that each contain both."""
    fx = Spans(55, 1200, 8, [(5 * w, 30, 1) for w in range(6)])
    present = np.ones((fx.nb, fx.K), bool)
    pairs = [(25, 26), (25, 29), (26, 28), (27, 28), (28, 29), (25, 27), (26, 29), (27, 29)]
    for b, (x, y) in enumerate(pairs):
        present[b, [x, y]] = False
    rpresent = np.ones((fx.nb, fx.R), bool)
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, pack(present), pack(rpresent))
    assert (s.status == RECOVERED).all() and (s.det == s.miss).all()
    assert not model.windows_alone(s, fx.off, fx.nss, propagate=True).any()
    rep = fx.encode(eng)
    work = np.where(s.miss[:, :, None], np.uint8(MISSING), fx.src)
    for w in range(6):  # the existing decode, one window at a time
        o = 5 * w
        blk = to_dev(work[:, o:o + 30])
        out = new_out(fx.nb)
        eng.rlc_decode_full(blk, to_dev(rep[:, w:w + 1]), to_dev(pack(present[:, o:o + 30])),
                            to_dev(pack(np.ones((fx.nb, 1), bool))), *out, 30, 1, fx.L, nblocks=fx.nb,
                            rep_seed=to_dev(np.zeros((fx.nb, 1), np.uint32)))
        torch.cuda.synchronize()
        st, rec = host_out(out)
        assert (st != RECOVERED).all() and not rec.any()
        assert np.array_equal(blk.cpu().numpy(), work[:, o:o + 30])
    _, _, _, got, st, _ = run_packed(eng, model, fx, present, rpresent)
    assert (st == RECOVERED).all() and np.array_equal(got, fx.src)


# --------------------------------------------------------------------------------- 2. equivalence with full-rank mode
@pytest.mark.parametrize("K,R,e", [(16, 6, 4), (64, 16, 16)])
def test_full_width_repairs_equal_full_rank_mode(eng, model, K, R, e):
    """Every repair covers the whole span: wherever fecgpu_rlc_decode_full recovers (or has no loss or no
    repair), status, recovered[] and bytes are identical."""
    nb, L = 4100, 64
    fx = Spans(K, L, nb, [(0, K, R)], data_seed=K)
    rng = np.random.default_rng([K, R, e])
    present = np.ones((nb, K), bool)
    for b in range(nb):
        present[b, rng.choice(K, e, replace=False)] = False
    rpresent = rng.random((nb, R)) < (0.85 if R == 6 else 0.97)
    present[:40] = True        # n == 0
    rpresent[40:80] = False    # m == 0
    s, work, rep_w, got, st, rec = run_packed(eng, model, fx, present, rpresent)
    full, part, none = coverage(s)
    assert full.sum() >= 1000 and part.sum() + none.sum() >= 100 and (s.status == NOTHING).sum() == 80
    # full-rank mode on the unpoisoned repairs (it may read any present one)
    rep_f = np.where(rpresent[:, :, None], fx.encode(eng), np.uint8(UNUSED))
    w = to_dev(work)
    out = new_out(nb)
    eng.rlc_decode_full(w, to_dev(rep_f), to_dev(pack(present)), to_dev(pack(rpresent)), *out, K, R, L, nblocks=nb,
                        rep_seed=to_dev(fx.seed))
    torch.cuda.synchronize()
    st_f, rec_f = host_out(out)
    n, m = (~present).sum(1), rpresent.sum(1)
    same = (st_f == RECOVERED) | (n == 0) | (m == 0)
    assert (st_f == RECOVERED).sum() >= 1000 and same.sum() >= 1080
    assert np.array_equal(st[same], st_f[same])
    assert np.array_equal(rec[same], rec_f[same])
    assert np.array_equal(got[same], w.cpu().numpy()[same])


# --------------------------------------------------------------------------------- 3. partial recovery
def test_partial_recovery_and_status_rules(eng, model):
    fx = Spans(60, 1200, 6, [(0, 30, 2), (30, 30, 2)])
    present = np.ones((fx.nb, fx.K), bool)
    rpresent = np.ones((fx.nb, fx.R), bool)
    present[0, [3, 17, 31, 40, 59]] = False  # cluster one: two repairs for two losses; cluster two: two for three
    present[1, [31, 40, 59]] = False         # no determined column
    present[2, [3, 17, 45]] = False          # both clusters determined
    present[4, [5, 50]] = False              # no repair received
    rpresent[4] = False
    present[5, [0, 29, 30]] = False          # one repair per cluster left: neither 2-loss cluster... one is
    rpresent[5, [1, 2]] = False
    s, work, _, got, st, _ = run_packed(eng, model, fx, present, rpresent)
    assert st.tolist() == [RECOVERED, SINGULAR, RECOVERED, NOTHING, NOTHING, RECOVERED]
    assert np.nonzero(s.det[0])[0].tolist() == [3, 17]
    assert np.nonzero(s.det[2])[0].tolist() == [3, 17, 45]
    assert np.nonzero(s.det[5])[0].tolist() == [30]
    assert (got[1] == work[1]).all() and (got[0, [31, 40, 59]] == MISSING).all()


# --------------------------------------------------------------------------------- 4. shapes
def _shape_case(name):
    """(spans, present, rpresent, off, nss) of a named shape; the loss patterns are fixed here."""
    off = nss = None
    if name in ("K70", "K128"):  # second mask word, pivots >= 64
        K = 70 if name == "K70" else 128
        fx = Spans(K, 64, 300, [(10 * w, 30, 2) for w in range((K - 30) // 10 + 1)] + [(K - 8, 8, 2)], data_seed=K)
        present, rpresent = random_losses(fx, [4, K], 0.07, 0.1)
        present[:20, 64:] = np.random.default_rng(K).random((20, K - 64)) >= 0.5
        present[299], rpresent[299] = True, True  # 35 losses in a row under eight repairs: nothing determined
        present[299, :35] = False
    elif name == "wide":  # n + K around 128 and 192: the third and fourth column registers
        fx = Spans(100, 64, 9, [(0, 100, 60), (0, 50, 20), (50, 50, 20)], data_seed=5)
        present = np.ones((fx.nb, fx.K), bool)
        rpresent = np.ones((fx.nb, fx.R), bool)
        rng = np.random.default_rng(100)
        for b, n in enumerate([28, 29, 30, 92, 93, 94, 100, 93, 29]):
            present[b, rng.choice(100, n, replace=False)] = False
        rpresent[7, 10:] = False  # 93 losses, 10 repairs
        rpresent[8, :60] = False  # 29 losses, the half-span repairs only
    elif name == "more_losses_than_slots":  # n > min(K, R), some still determined
        fx = Spans(40, 1200, 4, [(0, 8, 2), (8, 32, 4)], data_seed=6)
        present = np.ones((fx.nb, fx.K), bool)
        rpresent = np.ones((fx.nb, fx.R), bool)
        present[0, [1, 6] + list(range(10, 18))] = False        # n = 10, R = 6
        present[1, [2] + list(range(8, 40))] = False            # n = 33
        present[2, list(range(0, 8)) + [20, 21, 22, 23]] = False  # first cluster lost whole, second solvable
        present[3, list(range(40))] = False                     # everything lost
    elif name == "K128_R128":
        fx = Spans(128, 64, 4, [(0, 128, 64), (0, 64, 32), (64, 64, 32)], data_seed=7)
        present = np.ones((fx.nb, fx.K), bool)
        rpresent = np.ones((fx.nb, fx.R), bool)
        rng = np.random.default_rng(128)
        for b, n in enumerate([40, 100, 128, 40]):
            present[b, rng.choice(128, n, replace=False)] = False
        rpresent[3, :64] = False
        rpresent[3, 64:96] = rng.random(32) < 0.25
    elif name == "descriptors":
        # nss = 1, windows touching column 0 and K - 1, a window without losses, two identical repairs,
        # invalid descriptors on present repairs
        K = 24
        fx = Spans(K, 1200, 8, [(0, 1, 1), (K - 1, 1, 1), (0, 12, 1), (0, 12, 1), (12, 12, 2), (6, 12, 1), (4, 1, 1),
                                (8, 10, 1), (2, 20, 1)], data_seed=8)
        present = np.ones((fx.nb, fx.K), bool)
        rpresent = np.ones((fx.nb, fx.R), bool)
        present[0, [0, K - 1]] = False           # the one-symbol windows at both ends
        present[1, [1, 2]] = False               # the two identical repairs count once: (2, 20) is the second
        present[2, [13, 20]] = False             # windows (0, 12) hold no missing column
        present[3, [0, 4, 23]] = False
        present[4, [4, 9, 14]] = False
        present[5, [9, 14, 15, 16]] = False
        present[6, [3, 5]] = False
        present[7, [3, 5]] = False
        off, nss = fx.off.copy(), fx.nss.copy()
        nss[6, 2] = 0                            # an empty window on a present repair
        off[6, 3] = 20                           # leaves the span: 20 + 12 > 24 (span 7: the same losses, all valid)
    else:
        raise KeyError(name)
    return fx, present, rpresent, off, nss


@pytest.mark.parametrize("name", ["K70", "K128", "wide", "more_losses_than_slots", "K128_R128", "descriptors"])
def test_shapes(eng, model, name):
    fx, present, rpresent, off, nss = _shape_case(name)
    s, _, _, _, st, _ = run_packed(eng, model, fx, present, rpresent, off, nss)
    full, part, none = coverage(s)
    if name in ("K70", "K128"):
        assert full.any() and part.any() and none.any()
        piv64 = s.det[:, 64:].any(1)
        assert piv64.sum() >= 5
    elif name == "wide":
        n = s.miss.sum(1)
        assert n.tolist() == [28, 29, 30, 92, 93, 94, 100, 93, 29]
        assert full[:7].all() and not full[7] and s.det[8].any()
    elif name == "more_losses_than_slots":
        n = s.miss.sum(1)
        assert (n > fx.R).all()
        assert s.det.sum(1).tolist()[:2] == [2, 1] and s.det[2].sum() == 4 and st[3] == SINGULAR
    elif name == "K128_R128":
        assert full[:3].all() and s.det[2].sum() == 128 and part[3]
    else:
        assert s.det[0].tolist() == (~present[0]).tolist()
        assert s.selected[1, 2] and not s.selected[1, 3] and s.selected[1, 9] and full[1]
        assert not s.selected[2, 2] and not s.selected[2, 3]
        assert not s.valid[6, 2] and not s.valid[6, 3] and s.valid[7].all()
        assert s.det[7].sum() == 2 and st[6] == SINGULAR  # what the invalid descriptors cost


@pytest.mark.parametrize("e", [1, 2, 3, 4, 8, 16, 17])
def test_every_decode_tile(eng, model, e):
    """min(K, R) picks the data pass's tile (1, 2, 4, 8, 16); 17 unknowns take two passes and the finalize
    kernel.  Half of the spans lose e sources, the others fewer or more."""
    R = 20 if e == 17 else e
    fx = Spans(40, 1200, 12, [(0, 40, R)], data_seed=e)
    rng = np.random.default_rng(e)
    present = np.ones((fx.nb, fx.K), bool)
    for b in range(fx.nb):
        n = e if b % 2 == 0 else int(rng.integers(1, R + 3))
        present[b, rng.choice(40, n, replace=False)] = False
    rpresent = np.ones((fx.nb, fx.R), bool)
    rpresent[1::4, 0] = False
    s, _, _, _, _, _ = run_packed(eng, model, fx, present, rpresent)
    assert (s.det.sum(1)[::2] == e).all()


@pytest.fixture(scope="module")
def random_set(model):
    """3000 spans of k30 r1 step 5 under random loss, ordered so that every prefix used below holds what it
    can: span 0 is partially determined, the first three are one of each kind."""
    fx = Spans(55, 4, 3000, [(5 * w, 30, 1) for w in range(6)], data_seed=11)
    present, rpresent = random_losses(fx, 2026, 0.08, 0.15)
    s = model.solve(fx.K, fx.seed, fx.off, fx.nss, pack(present), pack(rpresent))
    full, part, none = coverage(s)
    assert full.sum() >= 100 and part.sum() >= 20 and none.sum() >= 20
    first = [int(np.nonzero(x)[0][0]) for x in (part, full, none)]
    order = np.array(first + [b for b in range(fx.nb) if b not in first])
    return order, present, rpresent


@pytest.mark.parametrize("L,nb", [(4, 3000), (4, 1), (1200, 65), (2052, 1), (2052, 65), (1200, 1)])
def test_lengths_and_batch_sizes(eng, model, random_set, L, nb):
    order, present, rpresent = random_set
    fx = Spans(55, L, nb, [(5 * w, 30, 1) for w in range(6)], data_seed=L)
    pick = order[:nb]
    s, _, _, _, _, _ = run_packed(eng, model, fx, present[pick], rpresent[pick])
    full, part, none = coverage(s)
    assert part[0] and (nb < 3 or (full[1] and none[2]))


# --------------------------------------------------------------------------------- 5. row forms
GAP = 8


def _ragged_set(eng, model):
    """Spans with ragged symbols: blk_len of every residue mod 4, sources cut to their own length, repairs
    as long as the longest source of their window."""
    K, L, nb = 55, 1200, 48
    fx = Spans(K, L, nb, [(5 * w, 30, 1) for w in range(6)], data_seed=21)
    rng = np.random.default_rng(21)
    blk = rng.integers(1, L + 1, nb)
    blk[:8] = [1, 2, 3, 5, 6, 7, L, L - 1]
    src_len = rng.integers(0, blk[:, None] + 1, (nb, K))
    src_len[np.arange(nb), rng.integers(0, K, nb)] = blk
    fx.src[np.arange(L)[None, None, :] >= src_len[:, :, None]] = 0
    rep_len = np.stack([src_len[:, o:o + n].max(1) for o, n, r in fx.windows for _ in range(r)], 1)
    assert (rep_len < blk[:, None]).any()
    present, rpresent = random_losses(fx, 5, 0.07, 0.15)
    present[:8, 26] = False
    off, nss = fx.off.copy(), fx.nss.copy()
    nss[9, 1] = 0  # an invalid descriptor on a present repair
    rpresent[9, 1] = True
    s = model.solve(K, fx.seed, off, nss, pack(present), pack(rpresent))
    full, part, none = coverage(s)
    assert full.any() and part.any() and none.any()
    rep = fx.encode(eng)
    assert not rep[np.arange(L)[None, None, :] >= rep_len[:, :, None]].any()
    return fx, blk, src_len, rep_len, present, rpresent, off, nss, s, rep


class Pool:
    """The rows of a batch shuffled through one byte pool, 4-byte aligned, sentinel bytes between them.  Row x of
    the sources has room for room[x] bytes; every repair the decode must not read shares one poisoned row."""

    def __init__(self, fx, s, blk, src_len, rep_len, rep, seed):
        nb, K, R, L = fx.nb, fx.K, fx.R, fx.L
        room = np.where(s.miss, blk[:, None], src_len).reshape(-1)
        lens = np.concatenate([room, np.where(s.selected, rep_len, 0).reshape(-1), [L]])
        order = np.random.default_rng(seed).permutation(lens.size)
        self.off = np.zeros(lens.size, np.int64)
        o = 0
        for x in order:
            self.off[x] = o
            o += ((int(lens[x]) + 3) & ~3) + GAP
        self.bytes = np.full(o, SENTINEL, np.uint8)
        for b in range(nb):
            for j in range(K):
                x = b * K + j
                self.bytes[self.off[x]:self.off[x] + room[x]] = MISSING if s.miss[b, j] else fx.src[b, j, :room[x]]
            for i in range(R):
                x = nb * K + b * R + i
                if s.selected[b, i]:
                    self.bytes[self.off[x]:self.off[x] + rep_len[b, i]] = rep[b, i, :rep_len[b, i]]
        self.bytes[self.off[-1]:self.off[-1] + L] = UNUSED
        self.srow = self.off[:nb * K].copy()
        self.rrow = np.where(s.selected.reshape(-1), self.off[nb * K:-1], self.off[-1])
        # what the pool holds afterwards: every determined source's blk_len bytes, nothing else changed
        self.want = self.bytes.copy()
        for b, j in zip(*np.nonzero(s.det)):
            o = self.off[b * K + j]
            self.want[o:o + blk[b]] = fx.src[b, j, :blk[b]]

    def tables(self, base):
        return (self.srow + base).astype(np.uint64), (self.rrow + base).astype(np.uint64)


def test_row_forms(eng, model):
    from pquic_amd import HostPath
    fx, blk, src_len, rep_len, present, rpresent, off, nss, s, rep = _ragged_set(eng, model)
    nb, K, R, L = fx.nb, fx.K, fx.R, fx.L
    sp, rp = pack(present), pack(rpresent)
    # the packed form on the zero-padded rows
    work, rep_w = damaged(fx, rep, s)
    w = to_dev(work)
    out = new_out(nb)
    eng.rlc_span_decode(w, to_dev(rep_w), to_dev(fx.seed), to_dev(off), to_dev(nss), to_dev(sp), to_dev(rp), *out, K, R,
                        L)
    torch.cuda.synchronize()
    st_p, rec_p = host_out(out)
    got_p = w.cpu().numpy()
    check(model, fx, s, work, got_p, st_p, rec_p)
    p = Pool(fx, s, blk, src_len, rep_len, rep, 31)
    slen = np.where(s.miss, 0, src_len).astype(np.uint32).reshape(-1)
    rlen = np.where(s.selected, rep_len, L).astype(np.uint32).reshape(-1)  # the poisoned row counts for L bytes

    def verify(st, rec, got, what):
        assert np.array_equal(st, st_p) and np.array_equal(rec, rec_p), what
        assert np.array_equal(got, p.want), (what, np.flatnonzero(got != p.want)[:8])
        for b, j in zip(*np.nonzero(s.det)):  # the packed form's bytes
            o = p.off[b * K + j]
            assert np.array_equal(got[o:o + blk[b]], got_p[b, j, :blk[b]])

    pool = to_dev(p.bytes)
    srow, rrow = p.tables(pool.data_ptr())
    out = new_out(nb)
    eng.rlc_span_decode_rows_fused(to_dev(srow), to_dev(slen), to_dev(rrow), to_dev(rlen), to_dev(blk.astype(np.uint32)),
                                   to_dev(fx.seed), to_dev(off), to_dev(nss), to_dev(sp), to_dev(rp), *out, nb, K, R, L)
    torch.cuda.synchronize()
    verify(*host_out(out), pool.cpu().numpy(), "device tables")

    keep = []

    def arr(a, pin):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        if not pin:
            return a.copy()
        t = torch.from_numpy(a.copy()).pin_memory()
        keep.append(t)
        return t.numpy()

    for cfg in ("pinned", "mixed"):  # mixed: one pageable table among page-locked ones; both sliced
        hp = HostPath(0, 3, 1 << 18)  # 73 200 B per span: steps of three spans
        pool = to_dev(p.bytes)
        srow, rrow = p.tables(pool.data_ptr())
        a = [arr(srow, True), arr(slen, True), arr(rrow, True), arr(rlen, True), arr(blk.astype(np.uint32), True),
             arr(fx.seed, True), arr(off, True), arr(nss, cfg != "mixed"), arr(sp, True), arr(rp, True),
             arr(np.full(nb, 0xEE, np.uint8), True), arr(np.full((nb, 2), 0xFF, np.uint64), True)]
        hp.rlc_span_decode_rows_fused(*a, nb, K, R, L)
        torch.cuda.synchronize()
        verify(a[10], a[11].view(np.uint64).reshape(nb, 2), pool.cpu().numpy(), cfg)
        hp.close()


# --------------------------------------------------------------------------------- 6. plan and apply
def test_plan_then_apply_forms(eng, model, random_set):
    order, present, rpresent = random_set
    nb, L = 200, 1200
    fx = Spans(55, L, nb, [(5 * w, 30, 1) for w in range(6)], data_seed=61)
    pick = order[:nb]
    s, work, rep_w, got, st, rec = run_packed(eng, model, fx, present[pick], rpresent[pick])
    ws = eng.alloc_workspace(nb, fx.K, fx.R)
    sp, rp = pack(present[pick]), pack(rpresent[pick])
    eng.rlc_span_decode_plan(to_dev(fx.seed), to_dev(fx.off), to_dev(fx.nss), to_dev(sp), to_dev(rp), fx.K, fx.R, nb, ws)
    w, r = to_dev(work), to_dev(rep_w)
    # apply_to: the recovered rows into another buffer of src's layout
    dst = torch.full((nb, fx.K, L), SENTINEL, dtype=torch.uint8, device=DEV)
    out = new_out(nb)
    eng.rlc_decode_apply_to(w, r, dst, *out, fx.K, fx.R, L, nb, ws)
    torch.cuda.synchronize()
    st2, rec2 = host_out(out)
    assert np.array_equal(st2, st) and np.array_equal(rec2, rec)
    assert np.array_equal(w.cpu().numpy(), work)
    d = dst.cpu().numpy()
    assert np.array_equal(d[s.det], got[s.det]) and (d[~s.det] == SENTINEL).all()
    # apply_packed: row u of a span = its u-th determined source, ascending
    em = min(fx.K, fx.R)
    dst = torch.full((nb, em, L), SENTINEL, dtype=torch.uint8, device=DEV)
    out = new_out(nb)
    eng.rlc_decode_apply_packed(w, r, dst, *out, fx.K, fx.R, L, nb, ws)
    torch.cuda.synchronize()
    st3, rec3 = host_out(out)
    assert np.array_equal(st3, st) and np.array_equal(rec3, rec)
    d = dst.cpu().numpy()
    for b in range(nb):
        cols = np.nonzero(s.det[b])[0]
        assert np.array_equal(d[b, :cols.size], got[b, cols]), b
        assert (d[b, cols.size:] == SENTINEL).all(), b
