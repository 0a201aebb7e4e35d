"""The header's stream contract (include/fecgpu.h: "Every call is asynchronous and graph-capturable: no
allocation, no synchronisation inside"), checked for every device entry point that takes a `stream`.

Each row of ROWS runs one entry point (or the plan / apply pair it belongs to) on a side stream S
(torch.cuda.Stream(): non-blocking against the null stream) in two arrangements, and compares bytes, statuses
and masks with the CPU oracle or the span model exactly as the entry point's own test module does:

  late_inputs       everything the kernels read by value is stale when the call is made (payload a sentinel
                    byte, masks all ones, seeds / fbn / wrow / lengths 0), every output, workspace and scratch
                    buffer a sentinel; S holds a delay, then the device copies that put the real inputs in
                    place, then an event E, then the engine's launches.  The host must have run ahead of the
                    device (`not E.query()` after the last engine call, else the run fails as inconclusive).
                    A launch that left S reads stale inputs or its producer's sentinel scratch.
  busy_null_stream  the null stream holds a delay longer than the case; the call, the synchronisation and the
                    read-back use S only.  A launch that went to the null stream has not run by then.

Address tables hold their final addresses from the start (a stale address would be dereferenced).

The delay.  Host-side enqueue time of the slowest row on an MI355X (wall clock around the engine calls,
first run, lazy initialisation included): 0.07 ms (MEASURED_ENQUEUE_MS; every row lay between 0.01 and 0.07 ms).
The delays are LATE_MS = 30 ms on S and BUSY_MS = 80 ms on the null stream: far more than 5 x that time, because
the device copies that deliver the inputs and the read-back of a few MiB take milliseconds of their own.  The delay
kernel's clock is calibrated once per process with two events.

The same cases serve the concurrent-callers test at the end and tests/test_graph_capture_gpu.py."""
import ctypes as C
import os
import re
import threading
import time

import numpy as np
import pytest

import decode_full_cases as FC
import test_decode_full_gpu as FD
import test_rows_fused_gpu as RF
import test_rows_len_gpu as RL
import test_span_decode_gpu as SD
import test_window_rows_gpu as WR
import test_xor_rows_gpu as XR
from oracle_py import DEC_RECOVERED, DEC_REF_UB, Oracle, synth_bytes
from span_model import SpanModel, bits, pack
from test_frames import Hdr
from test_rows_len_gpu import to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PAY, SENT = 0x3C, 0xD7          # stale payload byte; sentinel of outputs, workspaces and scratch
MISSING, ABSENT = 0xA5, 0x5C    # rows of missing sources / absent repairs, as test_gpu_parity fills them
MEASURED_ENQUEUE_MS = 0.07      # slowest row (plan + apply_packed at k40 r20), see the docstring
LATE_MS, BUSY_MS = 30, 80
assert min(LATE_MS, BUSY_MS) >= 5 * MEASURED_ENQUEUE_MS


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
def model():
    return SpanModel()


_clock = {}


def delay_cycles(ms):
    """torch.cuda._sleep cycles for `ms` milliseconds, from one calibration run per process."""
    if "per_ms" not in _clock:
        n = 4_000_000
        torch.cuda._sleep(1000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(n)
        b.record()
        torch.cuda.synchronize()
        _clock["per_ms"] = n / max(a.elapsed_time(b), 1e-3)
    return int(ms * _clock["per_ms"])


# ------------------------------------------------------------------------------------------------ a case
class Case:
    """The device buffers of one call sequence.  inp(): an input read by value -- `live` is what the kernels
    read (its address is final), `real` a device copy of the true content, `stale` what it holds before.
    const(): address tables.  out(): outputs, workspaces and scratch, refilled with a sentinel before every run.
    run(stream) makes the engine calls; reads maps names to the tensors fetch() brings to the host; check(got)
    compares them with the expectation computed once, on the CPU, when the case was built."""

    def __init__(self, eng):
        self.eng, self.ins, self.outs, self.keep, self.reads = eng, [], [], [], {}
        self.run = self.check = None

    def inp(self, a, stale):
        real = to_dev(np.ascontiguousarray(a))
        live = torch.empty_like(real)
        self.ins.append((live, real, stale))
        return live

    def const(self, a):
        t = to_dev(np.ascontiguousarray(a))
        self.keep.append(t)
        return t

    def out(self, shape, dtype=None, fill=SENT):
        t = torch.empty(shape, dtype=dtype or torch.uint8, device=DEV)
        self.outs.append((t, fill))
        return t

    def verdict(self, nb):
        return self.out((nb,), fill=0xEE), self.out((nb, 2), torch.int64, -1)

    def workspace(self, nbytes):
        return self.out((max(int(nbytes), 16),))

    def stage(self, late):
        """On the current stream: sentinels into everything written, stale or real content into the inputs."""
        for t, v in self.outs:
            t.fill_(v)
        for live, real, stale in self.ins:
            if late:
                live.fill_(stale)
            else:
                live.copy_(real)

    def deliver(self):
        for live, real, _ in self.ins:
            live.copy_(real)

    def layout(self):
        """Every address table as (buffer, offset) pairs: what stays when another case of the shape is loaded."""
        bufs = [x[0] for x in self.ins] + [x[0] for x in self.outs]
        start = np.array([b.data_ptr() for b in bufs], np.int64)
        order = np.argsort(start)
        out = []
        for t in self.keep:
            a = t.cpu().numpy().astype(np.int64)
            i = order[np.searchsorted(start[order], a, side="right") - 1]
            out.append(np.where(a == 0, -1, i).tolist() + np.where(a == 0, 0, a - start[i]).tolist())
        return out

    def fetch(self):
        got = {}
        for name, t in self.reads.items():
            h = t.cpu().numpy()
            got[name] = h.view(np.uint64) if h.dtype == np.int64 else h
        return got


def lib_call(eng, name, *args):
    rc = getattr(eng.lib, name)(*args)
    assert rc == 0, (name, rc, eng.err())


def sp_(stream):
    return C.c_void_p(stream.cuda_stream)


def row_table(t, nrows, stride):
    return (t.data_ptr() + np.arange(nrows, dtype=np.int64) * stride).astype(np.uint64)


# ------------------------------------------------------------------------------------------------ RLC encode
def build_encode(eng, oracle, k, r, L, nb, fbn_array):
    c = Case(eng)
    rng = np.random.default_rng([k, r, L, nb])
    src_h = synth_bytes(nb * k * L, 1000 + k * r).reshape(nb, k, L)
    base = 0xFFFFF0 + k  # the 24-bit wrap lies inside the batch
    fbn_h = ((base + rng.permutation(nb)) & 0xFFFFFF).astype(np.uint32) if fbn_array else None
    src = c.inp(src_h, PAY)
    fbn = c.inp(fbn_h, 0) if fbn_array else None
    rep = c.out((nb, r, L))
    if fbn_array:
        want = np.stack([np.stack(oracle.rlc_encode_block(int(fbn_h[b]), list(src_h[b]), r)[1]) for b in range(nb)])
    else:
        want = oracle.rlc_encode_batch(src_h, r, base)
    c.run = lambda s: eng.rlc_encode(src, rep, k, r, L, fbn_base=0 if fbn_array else base, fbn=fbn, stream=s)
    c.reads = {"rep": rep, "src": src}

    def check(g):
        assert np.array_equal(g["rep"], want), np.argwhere(g["rep"] != want)[:4]
        assert np.array_equal(g["src"], src_h)
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------ RLC decode
class Packed:
    """A packed decode batch and the oracle's verdict on it (reference mode), as test_decode_vs_oracle builds it;
    e_min: every third block loses at least that many sources."""

    _made = {}

    def __init__(self, oracle, k, r, L, nb, e_min=0, variant=0):
        rng = np.random.default_rng([k, r, L, nb, 7, variant])
        self.k, self.r, self.L, self.nb = k, r, L, nb
        self.src = synth_bytes(nb * k * L, 77 + k + 1000 * variant).reshape(nb, k, L)
        self.base = int(np.random.default_rng([k, r, L, nb]).integers(0, 1 << 24))  # a call argument: one per shape
        self.fbn = ((self.base + np.arange(nb)) & 0xFFFFFF).astype(np.uint32)
        self.seeds = ((self.fbn[:, None].astype(np.uint64) << 8) | np.arange(r, dtype=np.uint64)).astype(np.uint32)
        self.rep = oracle.rlc_encode_batch(self.src, r, self.base)
        self.present = np.ones((nb, k), bool)
        self.rpresent = np.zeros((nb, r), bool)
        em = min(k, r)
        for b in range(nb):
            e = int(rng.integers(max(e_min, 1), em + 1)) if b % 3 == 0 else int(rng.integers(0, em + 1))
            self.present[b, rng.choice(k, e, replace=False)] = False
            nrep = r if b % 3 == 0 else int(rng.integers(max(0, e - 1), r + 1))  # sometimes one repair short
            self.rpresent[b, rng.choice(r, nrep, replace=False)] = True
        self.sp, self.rp = pack(self.present), pack(self.rpresent)
        self.work = np.where(self.present[:, :, None], self.src, np.uint8(MISSING))
        self.repw = np.where(self.rpresent[:, :, None], self.rep, np.uint8(ABSENT))  # never read
        ref = self.work.copy()
        self.st, self.rec = oracle.rlc_decode_batch(ref, self.rep, self.sp, self.rp, self.base)
        self.recb = bits(self.rec, k)
        assert np.array_equal(ref[self.recb], self.src[self.recb])
        self.free = ~self.present & ~self.recb  # missing slots whose bit stays clear: unspecified bytes
        self.missing = [np.flatnonzero(~self.present[b]) for b in range(nb)]

    @classmethod
    def get(cls, oracle, *shape, **kw):
        key = shape + tuple(kw.items())
        if key not in cls._made:
            cls._made[key] = cls(oracle, *shape, **kw)
        return cls._made[key]

    def check_verdict(self, g):
        assert np.array_equal(g["st"], self.st), np.flatnonzero(g["st"] != self.st)[:8]
        assert np.array_equal(g["rec"], self.rec), np.flatnonzero((g["rec"] != self.rec).any(1))[:8]

    def check_in_place(self, rows):
        want = np.where(self.recb[:, :, None], self.src, self.work)
        rows = np.where(self.free[:, :, None], want, rows)
        assert np.array_equal(rows, want), np.argwhere((rows != want).any(2))[:8]

    def check_dst(self, dst):
        want = np.where(self.recb[:, :, None], self.src, np.uint8(SENT))
        free = self.free & (self.st == DEC_RECOVERED)[:, None]  # the data pass may have written these
        dst = np.where(free[:, :, None], want, dst)
        assert np.array_equal(dst, want), np.argwhere((dst != want).any(2))[:8]

    def check_packed(self, dst):
        for b in range(self.nb):
            m = self.missing[b]
            for u, j in enumerate(m):
                if self.recb[b, j]:
                    assert np.array_equal(dst[b, u], self.src[b, j]), (b, u, j)
            assert (dst[b, len(m):] == SENT).all(), b


def build_decode(eng, oracle, k, r, L, nb, form, e_min=0, variant=0):
    p = Packed.get(oracle, k, r, L, nb, e_min=e_min, variant=variant)
    if e_min > 16:
        over = ((~p.present).sum(1) > 16) & (p.st == DEC_RECOVERED)
        assert over.sum() >= 5, "the batch holds blocks with more than 16 unknowns that are recovered"
    assert (p.st == DEC_RECOVERED).sum() >= nb // 3
    c = Case(eng)
    work, rep = c.inp(p.work, PAY), c.inp(p.repw, PAY)
    sp, rp = c.inp(p.sp, -1), c.inp(p.rp, -1)
    fbn, seeds = c.inp(p.fbn, 0), c.inp(p.seeds, 0)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, k, r))
    em = min(k, r)
    dst = c.out((nb, em if form.endswith("packed") else k, L)) if "_to" in form or form.endswith("packed") else None
    a = lambda t: t.data_ptr()  # noqa: E731

    def plan(s):
        if form.startswith("seeded"):
            lib_call(eng, "fecgpu_rlc_decode_plan_seeded", nb, k, r, a(seeds), a(sp), a(rp), a(ws), ws.numel(), sp_(s))
        else:
            eng.rlc_decode_plan(sp, rp, k, r, nb, ws, fbn=fbn, stream=s)

    def run(s):
        if form == "decode":
            eng.rlc_decode(work, rep, sp, rp, st, rec, k, r, L, fbn=fbn, workspace=ws, stream=s)
        elif form == "seeded_decode":
            eng.rlc_decode_seeded(work, rep, seeds, sp, rp, st, rec, k, r, L, workspace=ws, stream=s)
        elif form == "rows":
            lib_call(eng, "fecgpu_rlc_decode_rows", a(srow), a(rrow), nb, k, r, L, a(seeds), a(sp), a(rp), a(st),
                     a(rec), a(ws), ws.numel(), sp_(s))
        else:
            plan(s)
            if form.endswith("apply"):
                eng.rlc_decode_apply(work, rep, st, rec, k, r, L, nb, ws, stream=s)
            elif form.endswith("apply_to"):
                eng.rlc_decode_apply_to(work, rep, dst, st, rec, k, r, L, nb, ws, stream=s)
            else:
                eng.rlc_decode_apply_packed(work, rep, dst, st, rec, k, r, L, nb, ws, stream=s)
    if form == "rows":
        srow, rrow = c.const(row_table(work, nb * k, L)), c.const(row_table(rep, nb * r, L))
    c.run = run
    c.reads = {"st": st, "rec": rec, "work": work, "rep": rep}
    if dst is not None:
        c.reads["dst"] = dst

    def check(g):
        p.check_verdict(g)
        assert np.array_equal(g["rep"], p.repw)
        if dst is None:
            p.check_in_place(g["work"])
        else:
            assert np.array_equal(g["work"], p.work), "src is only read"
            (p.check_packed if form.endswith("packed") else p.check_dst)(g["dst"])
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------ full-rank mode
_full = {}


def full_batch(k, r, L, nb, variant=0):
    """nb blocks of one decode_full_cases batch, chosen so that at least 10 are blocks the reference gives up on
    (REF_UB) and full mode recovers; block b keeps its block number idx[b]."""
    if (k, r, L, nb, variant) not in _full:
        big = FC.case(k, r, 6, 8, 2048, 21 + variant, L)
        gives_up = np.flatnonzero((big.ref_st == DEC_REF_UB) & big.full)
        assert gives_up.size >= 10, gives_up.size
        first = np.concatenate([gives_up[:20], np.flatnonzero(~big.full)[:5]])
        idx = np.concatenate([first, np.setdiff1d(np.arange(big.nb), first)])[:nb]
        assert ((big.ref_st[idx] == DEC_REF_UB) & big.full[idx]).sum() >= 10
        sub = FC.Case()
        sub.k, sub.r, sub.L, sub.nb = k, r, L, nb
        sub.idx, sub.src, sub.rep, sub.sp, sub.rp, sub.full = idx, big.src[idx], big.rep[idx], big.sp[idx], big.rp[idx], big.full[idx]
        sub.miss, sub.present = [big.miss[b] for b in idx], [big.present[b] for b in idx]
        sub.work, sub.repw = FC.damaged(sub)
        _full[(k, r, L, nb, variant)] = sub
    return _full[(k, r, L, nb, variant)]


def build_full(eng, oracle, k, r, L, nb, form, variant=0):
    f = full_batch(k, r, L, nb, variant)
    c = Case(eng)
    work, rep = c.inp(f.work, PAY), c.inp(f.repw, PAY)
    sp, rp = c.inp(f.sp, -1), c.inp(f.rp, -1)
    fbn = c.inp(f.idx.astype(np.uint32), 0)
    seeds = c.inp(((f.idx[:, None].astype(np.uint64) << 8) | np.arange(r, dtype=np.uint64)).astype(np.uint32), 0)
    slen, rlen, blen = (c.inp(np.full(n, L, np.uint32), 0) for n in (nb * k, nb * r, nb))
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, k, r))
    srow, rrow = c.const(row_table(work, nb * k, L)), c.const(row_table(rep, nb * r, L))

    def run(s):
        if form == "plan_full+apply":
            eng.rlc_decode_plan_full(sp, rp, k, r, nb, ws, fbn=fbn, stream=s)
            eng.rlc_decode_apply(work, rep, st, rec, k, r, L, nb, ws, stream=s)
        elif form == "decode_full":
            eng.rlc_decode_full(work, rep, sp, rp, st, rec, k, r, L, fbn=fbn, workspace=ws, stream=s)
        elif form == "decode_full_seeded":
            eng.rlc_decode_full(work, rep, sp, rp, st, rec, k, r, L, rep_seed=seeds, workspace=ws, stream=s)
        elif form == "rows_full":
            eng.rlc_decode_rows_full(srow, rrow, seeds, sp, rp, st, rec, nb, k, r, L, workspace=ws, stream=s)
        else:
            eng.rlc_decode_rows_fused_full(srow, slen, rrow, rlen, blen, seeds, sp, rp, st, rec, nb, k, r, L,
                                           workspace=ws, stream=s)
    c.run = run
    c.reads = {"st": st, "rec": rec, "work": work, "rep": rep}

    def check(g):
        FD.check_full(f, f.work, g["work"], g["st"], g["rec"], f.full)
        assert np.array_equal(g["rep"], f.repw)
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------ rows by address
def build_encode_rows(eng, oracle, k, r, L, nb):
    c = Case(eng)
    src_h = synth_bytes(nb * k * L, 900 + k).reshape(nb, k, L)
    rng = np.random.default_rng([k, r, nb, 3])
    fbn_h = rng.integers(0, 1 << 24, nb).astype(np.uint32)
    src, fbn = c.inp(src_h, PAY), c.inp(fbn_h, 0)
    rep = c.out((nb, r, L + 4))  # four guard bytes behind every repair row
    srow, rrow = c.const(row_table(src, nb * k, L)), c.const(row_table(rep, nb * r, L + 4))
    want = np.full((nb, r, L + 4), SENT, np.uint8)
    for b in range(nb):
        want[b, :, :L] = np.stack(oracle.rlc_encode_block(int(fbn_h[b]), list(src_h[b]), r)[1])
    c.run = lambda s: eng.rlc_encode_rows(srow, rrow, nb, k, r, L, fbn=fbn, stream=s)
    c.reads = {"rep": rep}
    c.check = lambda g: np.testing.assert_array_equal(g["rep"], want)
    return c


def build_ragged_encode(eng, oracle, k, r, L, nb, form):
    rng = np.random.default_rng([RF.SEED, k, r, nb])
    g, fbn_h, pool_h, want = RL._encode_case(rng, oracle, nb, k, r, L)
    c = Case(eng)
    pool = c.inp(pool_h, PAY)
    rows_s, src_len, rows_r, blk = RL._encode_tables(g, pool.data_ptr())
    rows_s, rows_r = c.const(rows_s), c.const(rows_r)
    src_len, blk, fbn = c.inp(src_len, 0), c.inp(blk, 0), c.inp(fbn_h, 0)
    ws = c.workspace(eng.rows_len_workspace_bytes(nb, k, r, L)) if form == "len" else None

    def run(s):
        if form == "len":
            eng.rlc_encode_rows_len(rows_s, src_len, rows_r, blk, nb, k, r, L, fbn=fbn, workspace=ws, stream=s)
        else:
            eng.rlc_encode_rows_fused(rows_s, src_len, rows_r, blk, nb, k, r, L, fbn=fbn, stream=s)
    c.run = run
    c.reads = {"pool": pool}
    c.check = lambda got: np.testing.assert_array_equal(got["pool"], want)
    return c


def build_ragged_decode(eng, oracle, k, r, L, nb, form):
    rng = np.random.default_rng([RF.SEED, k, r, nb, 1])
    d = RL.DecodeCase(rng, oracle, nb, k, r, L) if form == "len" else RF.FusedDecodeCase(rng, oracle, nb, k, r, L)
    n_rec = int((d.status == DEC_RECOVERED).sum())
    assert 2 * n_rec >= nb, n_rec
    c = Case(eng)
    pool = c.inp(d.pool_h, PAY)
    t = d.tables(pool.data_ptr())
    rows_s, rows_r = c.const(t[0]), c.const(t[2])
    slen, rlen, blen, seeds = (c.inp(t[i], 0) for i in (1, 3, 4, 5))
    sp, rp = c.inp(t[6], -1), c.inp(t[7], -1)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.rows_len_workspace_bytes(nb, k, r, L) if form == "len" else eng.decode_workspace_bytes(nb, k, r))
    call = eng.rlc_decode_rows_len if form == "len" else eng.rlc_decode_rows_fused
    c.run = lambda s: call(rows_s, slen, rows_r, rlen, blen, seeds, sp, rp, st, rec, nb, k, r, L, workspace=ws, stream=s)
    c.reads = {"pool": pool, "st": st, "rec": rec}
    chk = RL._check_decode if form == "len" else RF.check_decode
    c.check = lambda g: chk(d, g["pool"], g["st"], g["rec"], form)
    return c


def build_gather(eng, oracle, L, nrows):
    rng = np.random.default_rng([L, nrows])
    lens = RL._lens_for(L, nrows)
    p, off = RL._pool_rows(L, nrows)
    pool_h = rng.integers(1, 256, p.end + 64, dtype=np.uint8)
    c = Case(eng)
    pool = c.inp(pool_h, PAY)
    rows = (pool.data_ptr() + off).astype(np.uint64)
    rows[lens == 0] = 0
    rows, d_len = c.const(rows), c.inp(lens, 0)
    dst = c.out((nrows + 1, L))
    want = np.zeros((nrows + 1, L), np.uint8)
    want[nrows] = SENT
    for x in range(nrows):
        want[x, :lens[x]] = pool_h[off[x]:off[x] + lens[x]]
    c.run = lambda s: eng.rows_gather(rows, d_len, nrows, L, dst, stream=s)
    c.reads = {"dst": dst, "pool": pool}

    def check(g):
        assert np.array_equal(g["dst"], want), np.argwhere(g["dst"] != want)[:4]
        assert np.array_equal(g["pool"], pool_h)
    c.check = check
    return c


def build_scatter(eng, oracle, L, nrows):
    rng = np.random.default_rng([L, nrows, 1])
    lens = RL._lens_for(L, nrows)
    p, off = RL._pool_rows(L, nrows)
    src_h = rng.integers(0, 256, (nrows, L), dtype=np.uint8)
    c = Case(eng)
    pool = c.inp(p.bytes(), PAY)
    src, d_len = c.inp(src_h, PAY), c.inp(lens, 0)
    rows = (pool.data_ptr() + off).astype(np.uint64)
    rows[lens == 0] = 0
    rows = c.const(rows)
    want = p.bytes()
    for x in range(nrows):
        want[off[x]:off[x] + lens[x]] = src_h[x, :lens[x]]
    c.run = lambda s: eng.rows_scatter(src, rows, d_len, nrows, L, stream=s)
    c.reads = {"pool": pool}
    c.check = lambda g: np.testing.assert_array_equal(g["pool"], want)
    return c


# ------------------------------------------------------------------------------------------------ windows
def build_window(eng, oracle, k, r, step, L, nw, form):
    c = Case(eng)
    nsym = (nw - 1) * step + k
    sym_h = synth_bytes(nsym * L, 4242 + step).reshape(nsym, L)
    sym = c.inp(sym_h, PAY)
    wrow = c.inp((np.arange(nw) * step).astype(np.uint32), 0)
    rep = c.out((nw, r, L))
    want = np.stack([np.stack(oracle.rlc_encode_block(0, list(sym_h[w * step: w * step + k]), r)[1]) for w in range(nw)])

    def run(s):
        if form == "table":
            eng.rlc_window_encode_table(sym, nsym, wrow, rep, nw, k, r, L, stream=s)
        elif form == "sc0":
            with eng.knob("window_sc", 0):
                eng.rlc_window_encode(sym, rep, nw, step, k, r, L, stream=s)
        else:
            eng.rlc_window_encode(sym, rep, nw, step, k, r, L, stream=s)
    c.run = run
    c.reads = {"rep": rep}
    c.check = lambda g: np.testing.assert_array_equal(g["rep"], want)
    return c


class StepWindows(WR.Case):
    """test_window_rows_gpu.Case over windows a fixed step apart.  Its own layouts are 'overlap', 'adjacent' and
    'mixed', chosen by its module's starts(); that function is replaced for the time of the construction."""

    def __init__(self, oracle, S, k, r, step, nwin, seed):
        keep = WR.starts
        WR.starts = lambda kind, k_, n: [w * step for w in range(n)]
        try:
            super().__init__(oracle, S, k, r, "step", nwin, seed)
        finally:
            WR.starts = keep


def build_window_rows(eng, oracle, k, r, step, L, nw):
    w = StepWindows(oracle, L, k, r, step, nw, 31 * L + 7 * k + r + nw)
    assert w.longer and any(o is None for o in w.row_off)
    c = Case(eng)
    pool = c.inp(w.image, PAY)
    t = w.tables(pool.data_ptr())
    rows, rep_rows = c.const(t["rows"]), c.const(t["rep_rows"])
    row_len, wrow, blk_len = c.inp(t["row_len"], 0), c.inp(t["wrow"], 0), c.inp(t["blk_len"], 0)
    ws = c.workspace(eng.window_rows_workspace_bytes(w.nrows, L))
    c.run = lambda s: eng.rlc_window_encode_rows(rows, row_len, w.nrows, wrow, rep_rows, blk_len, nw, k, r, L,
                                                 workspace=ws, stream=s)
    c.reads = {"pool": pool}
    c.check = lambda g: np.testing.assert_array_equal(g["pool"], w.want)
    return c


# ------------------------------------------------------------------------------------------------ span decode
def span_set(eng, layout, ragged=False, variant=0):
    """multi: the layout and losses of test_rows_more_than_16_unknowns (17 to 21 losses per span: several tile
    launches and the finalize kernel); single: k30 r1 step 5 spans of 55 columns at 70 spans."""
    if layout == "multi":
        fx = SD.Spans(40, 1200, 12, [(0, 20, 10), (10, 30, 12)], data_seed=17 + variant)
        rng = np.random.default_rng(17 + variant)
        present = np.ones((fx.nb, fx.K), bool)
        for b in range(fx.nb):
            present[b, rng.choice(40, 17 + b % 5, replace=False)] = False
        rpresent = np.ones((fx.nb, fx.R), bool)
        rpresent[1::3, 4] = False
    else:
        fx = SD.Spans(55, 1200, 70, [(5 * w, 30, 1) for w in range(6)], data_seed=61)
        present, rpresent = SD.random_losses(fx, 61, 0.08, 0.15)
    lens = None
    if ragged:  # as test_span_decode_gpu._ragged_set: sources cut to their own length before the encode
        rng = np.random.default_rng(21 + variant)
        nb, K, L = fx.nb, fx.K, fx.L
        blk = rng.integers(1, L + 1, nb)
        src_len = rng.integers(0, blk[:, None] + 1, (nb, K))
        src_len[np.arange(nb), rng.integers(0, K, nb)] = blk
        fx.src[np.arange(L)[None, None, :] >= src_len[:, :, None]] = 0
        rep_len = np.stack([src_len[:, o:o + n].max(1) for o, n, r in fx.windows for _ in range(r)], 1)
        lens = (blk, src_len, rep_len)
    return fx, present, rpresent, fx.encode(eng), lens


def build_span(eng, model, layout, form):
    fx, present, rpresent, rep_h, _ = span_set(eng, layout)
    nb, K, R, L = fx.nb, fx.K, fx.R, fx.L
    sp_h, rp_h = pack(present), pack(rpresent)
    s = model.solve(K, fx.seed, fx.off, fx.nss, sp_h, rp_h)
    if layout == "multi":
        assert (s.det.sum(1) > 16).sum() >= 6
    else:
        assert (s.det.sum(1) > 0).sum() >= 20 and s.det.sum(1).max() <= 16
    work_h, rep_w = SD.damaged(fx, rep_h, s)
    c = Case(eng)
    work, rep = c.inp(work_h, PAY), c.inp(rep_w, PAY)
    seed, off, nss = c.inp(fx.seed, 0), c.inp(fx.off, 0), c.inp(fx.nss, 0)
    sp, rp = c.inp(sp_h, -1), c.inp(rp_h, -1)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, K, R))

    def run(t):
        if form == "span_decode":
            eng.rlc_span_decode(work, rep, seed, off, nss, sp, rp, st, rec, K, R, L, nspans=nb, workspace=ws, stream=t)
        else:
            eng.rlc_span_decode_plan(seed, off, nss, sp, rp, K, R, nb, ws, stream=t)
            eng.rlc_decode_apply(work, rep, st, rec, K, R, L, nb, ws, stream=t)
    c.run = run
    c.reads = {"st": st, "rec": rec, "work": work, "rep": rep}

    def check(g):
        SD.check(model, fx, s, work_h, g["work"], g["st"], g["rec"])
        assert np.array_equal(g["rep"], rep_w)
    c.check = check
    return c


def build_span_rows(eng, model, layout):
    fx, present, rpresent, rep_h, (blk, src_len, rep_len) = span_set(eng, layout, ragged=True)
    nb, K, R, L = fx.nb, fx.K, fx.R, fx.L
    sp_h, rp_h = pack(present), pack(rpresent)
    s = model.solve(K, fx.seed, fx.off, fx.nss, sp_h, rp_h)
    if layout == "multi":
        assert (s.det.sum(1) > 16).sum() >= 6
    p = SD.Pool(fx, s, blk, src_len, rep_len, rep_h, 31)
    c = Case(eng)
    pool = c.inp(p.bytes, PAY)
    srow, rrow = p.tables(pool.data_ptr())
    srow, rrow = c.const(srow), c.const(rrow)
    slen = c.inp(np.where(s.miss, 0, src_len).astype(np.uint32).reshape(-1), 0)
    rlen = c.inp(np.where(s.selected, rep_len, L).astype(np.uint32).reshape(-1), 0)
    blen = c.inp(blk.astype(np.uint32), 0)
    seed, off, nss = c.inp(fx.seed, 0), c.inp(fx.off, 0), c.inp(fx.nss, 0)
    sp, rp = c.inp(sp_h, -1), c.inp(rp_h, -1)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, K, R))
    exp_rec = model.recovered(s, fx.src)
    c.run = lambda t: eng.rlc_span_decode_rows_fused(srow, slen, rrow, rlen, blen, seed, off, nss, sp, rp, st, rec, nb, K,
                                                     R, L, workspace=ws, stream=t)
    c.reads = {"st": st, "rec": rec, "pool": pool}

    def check(g):
        assert np.array_equal(g["st"], s.status) and np.array_equal(g["rec"], exp_rec)
        assert np.array_equal(g["pool"], p.want), np.flatnonzero(g["pool"] != p.want)[:8]
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------ XOR
def build_xor(eng, oracle, k, L, nb, form):
    rng = np.random.default_rng([k, L, nb, 9])
    src_h = synth_bytes(nb * k * L, k).reshape(nb, k, L)
    rep_h = oracle.xor_encode_batch(src_h)
    c = Case(eng)
    if form == "encode":
        src, rep = c.inp(src_h, PAY), c.out((nb, 1, L))
        c.run = lambda s: eng.xor_encode(src, rep, k, L, stream=s)
        c.reads = {"rep": rep}
        c.check = lambda g: np.testing.assert_array_equal(g["rep"], rep_h)
        return c
    present = np.ones((nb, k), bool)
    rpresent = rng.random((nb, 1)) < 0.8
    for b in range(nb):
        present[b, rng.choice(k, min(int(rng.integers(0, 3)), k), replace=False)] = False
    sp_h, rp_h = pack(present), pack(rpresent)
    work_h = np.where(present[:, :, None], src_h, np.uint8(MISSING))
    repw = np.where(rpresent[:, :, None], rep_h, np.uint8(ABSENT))
    ref = work_h.copy()
    st_ref, rec_ref = oracle.xor_decode_batch(ref, rep_h, sp_h, rp_h)
    ok = st_ref == DEC_RECOVERED
    assert ok.sum() >= nb // 8 and (~ok).sum() >= nb // 8 and np.array_equal(ref[ok], src_h[ok])
    work, rep = c.inp(work_h, PAY), c.inp(repw, PAY)
    sp, rp = c.inp(sp_h, -1), c.inp(rp_h, -1)
    st, rec = c.verdict(nb)
    dst = c.out((nb, L)) if form == "decode_to" else None

    def run(s):
        if dst is None:
            eng.xor_decode(work, rep, sp, rp, st, rec, k, L, stream=s)
        else:
            eng.xor_decode_to(work, rep, dst, sp, rp, st, rec, k, L, stream=s)
    c.run = run
    c.reads = {"st": st, "rec": rec, "work": work}
    if dst is not None:
        c.reads["dst"] = dst
    miss = np.argmax(~present, axis=1)

    def check(g):
        assert np.array_equal(g["st"], st_ref) and np.array_equal(g["rec"], rec_ref)
        if dst is None:
            assert np.array_equal(g["work"][ok], src_h[ok]) and np.array_equal(g["work"][~ok], work_h[~ok])
        else:
            assert np.array_equal(g["work"], work_h), "the received block was written"
            want = np.where(ok[:, None], src_h[np.arange(nb), miss], np.uint8(SENT))
            assert np.array_equal(g["dst"], want)
    c.check = check
    return c


def build_xor_rows(eng, oracle, k, L, nb, form):
    x = XR.EncodeCase(oracle, k, L, nb, 1000 * k + L + nb) if form == "encode" else XR.DecodeCase(oracle, k, L, nb, 31 * k + L + nb)
    c = Case(eng)
    pool = c.inp(x.image, PAY)
    rows, reps = x.tables(pool.data_ptr())
    rows, reps = c.const(rows), c.const(reps)
    slen, blen = c.inp(x.src_len, 0), c.inp(x.blk_len, 0)
    if form == "encode":
        c.run = lambda s: eng.xor_encode_rows(rows, slen, reps, blen, x.nb, k, L, stream=s)
        c.reads = {"pool": pool}
        c.check = lambda g: np.testing.assert_array_equal(g["pool"], x.want)
        return c
    assert {DEC_RECOVERED, DEC_REF_UB} <= set(x.st.tolist())
    sp, rp = c.inp(x.sp, -1), c.inp(x.rp, -1)
    st, rec = c.verdict(x.nb)
    c.run = lambda s: eng.xor_decode_rows(rows, slen, reps, blen, sp, rp, st, rec, x.nb, k, L, stream=s)
    c.reads = {"pool": pool, "st": st, "rec": rec}

    def check(g):
        assert np.array_equal(g["st"], x.st) and np.array_equal(g["rec"], x.rec)
        assert np.array_equal(g["pool"], x.want), np.flatnonzero(g["pool"] != x.want)[:8]
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------ frames, synth
def build_frames(eng, oracle, nb, r, L, dlen, stride):
    rng = np.random.default_rng(nb)
    rep_h = rng.integers(0, 256, (nb, r, L), dtype=np.uint8)
    fbn_h = rng.integers(0, 1 << 24, nb, dtype=np.uint32)
    c = Case(eng)
    rep, fbn = c.inp(rep_h, PAY), c.inp(fbn_h, 0)
    frames = c.out((nb * r, stride))
    lib = eng.lib
    lib.pquic_fec_write_fec_frame_header.argtypes = [C.POINTER(Hdr), C.POINTER(C.c_uint8)]
    lib.pquic_fec_write_fec_frame_header.restype = C.c_size_t
    want = np.zeros((nb * r, stride), np.uint8)
    for b in range(nb):
        for i in range(r):
            buf = (C.c_uint8 * 14)()
            lib.pquic_fec_write_fec_frame_header(C.byref(Hdr(1, dlen, 1, (int(fbn_h[b]) << 8) | i, 16, r)), buf)
            want[b * r + i, :14] = np.frombuffer(bytes(buf), np.uint8)
            want[b * r + i, 14:14 + dlen] = rep_h[b, i, :dlen]
    c.run = lambda s: eng.write_repair_frames(rep, frames, nb, r, L, dlen, stride, 16, r, fbn=fbn, stream=s)
    c.reads = {"frames": frames}
    c.check = lambda g: np.testing.assert_array_equal(g["frames"], want)
    return c


def build_synth(eng, oracle, nbytes, seed, off):
    c = Case(eng)
    buf = c.out((nbytes + 16,))
    want = np.concatenate([synth_bytes(nbytes, seed, off), np.full(16, SENT, np.uint8)])
    c.run = lambda s: eng.synth_fill(buf, nbytes, seed, off, stream=s)
    c.reads = {"buf": buf}
    c.check = lambda g: np.testing.assert_array_equal(g["buf"], want)
    return c


# ------------------------------------------------------------------------------------------------ the table
class Row:
    def __init__(self, name, entries, build, *args, model=False, **kw):
        self.id, self.entries, self.build, self.args, self.kw, self.model = name, entries, build, args, kw, model


def _decode_rows(shape, tag, **kw):
    forms = [("decode", ["rlc_decode"]), ("plan+apply", ["rlc_decode_plan", "rlc_decode_apply"]),
             ("plan+apply_to", ["rlc_decode_plan", "rlc_decode_apply_to"]),
             ("plan+apply_packed", ["rlc_decode_plan", "rlc_decode_apply_packed"]),
             ("seeded_decode", ["rlc_decode_seeded"]), ("seeded_plan+apply", ["rlc_decode_plan_seeded", "rlc_decode_apply"]),
             ("seeded_plan+apply_to", ["rlc_decode_plan_seeded", "rlc_decode_apply_to"]),
             ("seeded_plan+apply_packed", ["rlc_decode_plan_seeded", "rlc_decode_apply_packed"])]
    return [Row(f"{form}-{tag}", ent, build_decode, *shape, form, **kw) for form, ent in forms]


ROWS = [
    Row("encode-k5r17-two_tiles", ["rlc_encode"], build_encode, 5, 17, 300, 70, True),
    Row("encode-k16r4-nb7-lds", ["rlc_encode"], build_encode, 16, 4, 1200, 7, False),
    Row("encode-k9r16-ring_two_chunks", ["rlc_encode"], build_encode, 9, 16, 2052, 70, False),
    *_decode_rows((40, 20, 100, 70), "k40r20-over16", e_min=17),
    *_decode_rows((16, 4, 1200, 7), "k16r4-nb7"),
    Row("plan_full+apply-k16r8", ["rlc_decode_plan_full", "rlc_decode_apply"], build_full, 16, 8, 256, 100, "plan_full+apply"),
    Row("decode_full-k16r8", ["rlc_decode_full"], build_full, 16, 8, 256, 100, "decode_full"),
    Row("decode_full-seeded-k16r8", ["rlc_decode_full"], build_full, 16, 8, 256, 100, "decode_full_seeded"),
    Row("decode_rows_full-k16r8", ["rlc_decode_rows_full"], build_full, 16, 8, 256, 100, "rows_full"),
    Row("decode_rows_fused_full-k16r8", ["rlc_decode_rows_fused_full"], build_full, 16, 8, 256, 100, "rows_fused_full"),
    Row("encode_rows-k12r6", ["rlc_encode_rows"], build_encode_rows, 12, 6, 1204, 70),
    Row("decode_rows-k12r6", ["rlc_decode_rows"], build_decode, 12, 6, 1204, 70, "rows"),
    Row("encode_rows_fused-k12r6", ["rlc_encode_rows_fused"], build_ragged_encode, 12, 6, 1204, 70, "fused"),
    Row("decode_rows_fused-k12r6", ["rlc_decode_rows_fused"], build_ragged_decode, 12, 6, 1204, 70, "fused"),
    Row("encode_rows_len-k12r6", ["rlc_encode_rows_len"], build_ragged_encode, 12, 6, 1204, 70, "len"),
    Row("decode_rows_len-k12r6", ["rlc_decode_rows_len"], build_ragged_decode, 12, 6, 1204, 70, "len"),
    Row("rows_gather", ["rows_gather"], build_gather, 1204, 840),
    Row("rows_scatter", ["rows_scatter"], build_scatter, 1204, 840),
    Row("window_encode", ["rlc_window_encode"], build_window, 30, 5, 10, 1200, 40, "sc"),
    Row("window_encode-window_sc0", ["rlc_window_encode"], build_window, 30, 5, 10, 1200, 40, "sc0"),
    Row("window_encode_table", ["rlc_window_encode_table"], build_window, 30, 5, 10, 1200, 40, "table"),
    Row("window_encode_rows", ["rlc_window_encode_rows"], build_window_rows, 30, 5, 10, 1200, 40),
    Row("span_plan+apply-multi_tile", ["rlc_span_decode_plan", "rlc_decode_apply"], build_span, "multi", "plan+apply", model=True),
    Row("span_decode-multi_tile", ["rlc_span_decode"], build_span, "multi", "span_decode", model=True),
    Row("span_decode_rows_fused-multi_tile", ["rlc_span_decode_rows_fused"], build_span_rows, "multi", model=True),
    Row("span_plan+apply-single_tile", ["rlc_span_decode_plan", "rlc_decode_apply"], build_span, "single", "plan+apply", model=True),
    Row("span_decode-single_tile", ["rlc_span_decode"], build_span, "single", "span_decode", model=True),
    Row("span_decode_rows_fused-single_tile", ["rlc_span_decode_rows_fused"], build_span_rows, "single", model=True),
    *[Row(f"xor_{form}-k{k}", [f"xor_{form}"], build_xor, k, L, nb, form)
      for k, L, nb in ((4, 1200, 300), (7, 52, 70)) for form in ("encode", "decode", "decode_to")],
    *[Row(f"xor_{form}_rows-k{k}", [f"xor_{form}_rows"], build_xor_rows, k, L, nb, form)
      for k, L, nb in ((4, 1200, 300), (7, 52, 70)) for form in ("encode", "decode")],
    Row("write_repair_frames", ["write_repair_frames"], build_frames, 33, 8, 1200, 1000, 1216),
    Row("synth_fill", ["synth_fill"], build_synth, 4099, 7, 13),
]
BY_ID = {r.id: r for r in ROWS}
_built = {}


def built(row, eng, oracle, model):
    """The row's case: buffers and the CPU expectation, made once and shared by both arrangements."""
    if row.id not in _built:
        _built[row.id] = row.build(eng, model if row.model else oracle, *row.args, **row.kw)
        torch.cuda.synchronize()
    return _built[row.id]


ENQUEUE_MS = {}


def run_late_inputs(c, S, name=None):
    c.stage(late=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(delay_cycles(LATE_MS))
        c.deliver()
        E = torch.cuda.Event()
        E.record(S)
        t0 = time.perf_counter()
        c.run(S)
        ENQUEUE_MS[name] = (time.perf_counter() - t0) * 1e3
        ahead = not E.query()
    assert ahead, ("inconclusive: the device had caught up with the host when the last engine call returned "
                   f"(enqueue took {ENQUEUE_MS[name]:.2f} ms under a delay of {LATE_MS} ms)")
    S.synchronize()
    with torch.cuda.stream(S):
        got = c.fetch()
    c.check(got)


def run_busy_null_stream(c, S):
    with torch.cuda.stream(S):
        c.stage(late=False)
    S.synchronize()
    try:
        torch.cuda._sleep(delay_cycles(BUSY_MS))  # the current stream is the null stream
        E0 = torch.cuda.Event()
        E0.record()
        c.run(S)
        S.synchronize()
        with torch.cuda.stream(S):
            got = c.fetch()
        busy = not E0.query()
    finally:
        torch.cuda.synchronize()
    assert busy, f"inconclusive: the null stream's delay of {BUSY_MS} ms ended before the read-back"
    c.check(got)


@pytest.fixture(scope="module")
def side():
    """A side stream that runs beside the null stream.  HIP maps streams onto a few hardware queues (four by
    default); a stream that landed on the null stream's queue would run behind its delay, and the busy
    arrangement would prove nothing.  Candidates come from torch's pool in turn; each is probed once."""
    probe = torch.zeros(64, dtype=torch.uint8, device=DEV)
    for _ in range(16):
        S = torch.cuda.Stream()
        torch.cuda.synchronize()
        torch.cuda._sleep(delay_cycles(20))
        busy = torch.cuda.Event()
        busy.record()
        with torch.cuda.stream(S):
            probe.fill_(1)
        S.synchronize()
        beside = not busy.query()
        torch.cuda.synchronize()
        if beside:
            return S
    pytest.fail("inconclusive: none of 16 streams ran beside a busy null stream")


@pytest.mark.parametrize("arrangement", ["late_inputs", "busy_null_stream"])
@pytest.mark.parametrize("name", [r.id for r in ROWS])
def test_entry_point_on_a_side_stream(eng, oracle, model, side, name, arrangement):
    c = built(BY_ID[name], eng, oracle, model)
    assert torch.cuda.current_stream().cuda_stream == 0, "the tests' current stream is the null stream"
    if arrangement == "late_inputs":
        run_late_inputs(c, side, name)
        print(f"enqueue {name}: {ENQUEUE_MS[name]:.3f} ms")
    else:
        run_busy_null_stream(c, side)


def test_every_stream_entry_point_of_the_header_has_a_row():
    text = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bfecgpu_(\w+)\s*\(([^;{}]*?)\)\s*;", text)
    streamed = {name for name, args in protos if re.search(r"void\s*\*\s*stream\s*$", args.strip())}
    assert len(streamed) >= 33, sorted(streamed)
    covered = {e for r in ROWS for e in r.entries}
    assert streamed - covered == set(), f"no row for {sorted(streamed - covered)}"
    assert covered - streamed == set(), f"rows name no entry point of the header: {sorted(covered - streamed)}"


# ------------------------------------------------------------------------------------------------ concurrent callers
def test_concurrent_callers(eng, oracle, model):
    """The four call sequences of the engine's callers at once, each thread with its own stream, shape, buffers
    and workspace, released by a barrier: encode then decode; full-rank decode; span plan then apply_packed, on
    two threads (two workspaces, so the engine's record of the last span plan alternates between them); XOR
    rows.  ctypes drops the GIL around every engine call.  Every iteration's bytes, statuses and masks equal the
    expectation computed before the threads start, and fecgpu_last_error() stays empty on every thread; no knob
    is touched."""
    iters = 20
    p = Packed.get(oracle, 16, 4, 1200, 70)
    seqs = [[_encode_then_decode(eng, oracle, p)], [built(BY_ID["decode_full-k16r8"], eng, oracle, model)],
            [_span_packed(eng, model, "multi")], [_span_packed(eng, model, "single")],
            [built(BY_ID["xor_encode_rows-k4"], eng, oracle, model), built(BY_ID["xor_decode_rows-k4"], eng, oracle, model)]]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in seqs]
    barrier = threading.Barrier(len(seqs))
    failures = []

    def worker(t):
        try:
            torch.cuda.set_device(0)
            S = streams[t]
            barrier.wait()
            with torch.cuda.stream(S):
                for it in range(iters):
                    for c in seqs[t]:  # the whole sequence enqueued before the thread waits for any of it
                        c.stage(late=False)
                        c.run(S)
                    S.synchronize()
                    for c in seqs[t]:
                        c.check(c.fetch())
            err = eng.err()
            assert err == "", err
        except BaseException as e:  # noqa: BLE001
            failures.append((t, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(len(seqs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not failures, failures


def _encode_then_decode(eng, oracle, p):
    """rlc_encode, then plan and apply_packed on the repairs it wrote (the bench's path)."""
    k, r, L, nb = p.k, p.r, p.L, p.nb
    c = Case(eng)
    src, work = c.inp(p.src, PAY), c.inp(p.work, PAY)
    sp, rp = c.inp(p.sp, -1), c.inp(pack(np.ones((nb, r), bool)), -1)
    rep = c.out((nb, r, L))
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, k, r))
    dst = c.out((nb, min(k, r), L))
    ref = p.work.copy()
    st_ref, rec_ref = oracle.rlc_decode_batch(ref, p.rep, p.sp, pack(np.ones((nb, r), bool)), p.base)
    recb = bits(rec_ref, k)

    def run(s):
        eng.rlc_encode(src, rep, k, r, L, fbn_base=p.base, stream=s)
        eng.rlc_decode_plan(sp, rp, k, r, nb, ws, fbn_base=p.base, stream=s)
        eng.rlc_decode_apply_packed(work, rep, dst, st, rec, k, r, L, nb, ws, stream=s)
    c.run = run
    c.reads = {"rep": rep, "st": st, "rec": rec, "dst": dst}

    def check(g):
        assert np.array_equal(g["rep"], p.rep)
        assert np.array_equal(g["st"], st_ref) and np.array_equal(g["rec"], rec_ref)
        for b in range(nb):
            m = p.missing[b]
            for u, j in enumerate(m):
                if recb[b, j]:
                    assert np.array_equal(g["dst"][b, u], p.src[b, j]), (b, u, j)
            assert (g["dst"][b, len(m):] == SENT).all(), b
    c.check = check
    return c


def _span_packed(eng, model, layout):
    """fecgpu_rlc_span_decode_plan, then fecgpu_rlc_decode_apply_packed: row u = the u-th determined source."""
    fx, present, rpresent, rep_h, _ = span_set(eng, layout)
    nb, K, R, L = fx.nb, fx.K, fx.R, fx.L
    sp_h, rp_h = pack(present), pack(rpresent)
    s = model.solve(K, fx.seed, fx.off, fx.nss, sp_h, rp_h)
    work_h, rep_w = SD.damaged(fx, rep_h, s)
    exp_rec = model.recovered(s, fx.src)
    c = Case(eng)
    work, rep = c.inp(work_h, PAY), c.inp(rep_w, PAY)
    seed, off, nss = c.inp(fx.seed, 0), c.inp(fx.off, 0), c.inp(fx.nss, 0)
    sp, rp = c.inp(sp_h, -1), c.inp(rp_h, -1)
    st, rec = c.verdict(nb)
    ws = c.workspace(eng.decode_workspace_bytes(nb, K, R))
    em = min(K, R)
    dst = c.out((nb, em, L))

    def run(t):
        eng.rlc_span_decode_plan(seed, off, nss, sp, rp, K, R, nb, ws, stream=t)
        eng.rlc_decode_apply_packed(work, rep, dst, st, rec, K, R, L, nb, ws, stream=t)
    c.run = run
    c.reads = {"st": st, "rec": rec, "dst": dst, "work": work}

    def check(g):
        assert np.array_equal(g["st"], s.status) and np.array_equal(g["rec"], exp_rec)
        assert np.array_equal(g["work"], work_h)
        for b in range(nb):
            cols = np.flatnonzero(s.det[b])
            assert np.array_equal(g["dst"][b, :cols.size], fx.src[b, cols]), b
            assert (g["dst"][b, cols.size:] == SENT).all(), b
    c.check = check
    return c
