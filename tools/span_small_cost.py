"""What one span decode call on rows costs a synchronous caller at 1, 8 and 64 spans, this tree against a build
of the parent commit in one process (tools/build_at_commit.sh PARENT OUT.so), the variants alternating call by
call: K 30 R 6 (one window of 30 under 6 repairs) and K 125 R 20 (k30 r1 step 5, twenty windows), L 1200,
sources and repairs lost independently with p = 0.03.  A call is timed by the host clock from the call to the
end of a stream synchronise, which is what a blocking caller waits for; medians of --calls calls with min-max.
`plan1` is this tree with knob plan = 1 (the separate launches), a cross-check of the parent's figure only.
Every variant's status, recovered[] and rows must equal the first variant's.  Then, through tools/libspanload.so,
the blocking hook call pquic_fec_rlc_recover_span for one span of either shape: p50 / p99 / min of --hook-calls
draws of the losses (a draw without a lost source or without a repair is not a call).
(tools/lib_ab.py interleaves whole builds in the same way, two Engine objects on private loads of the two
libraries, but its cases are the bench's bulk shapes; this tool keeps that scheme and brings its own cases.)
usage: python tools/span_small_cost.py --parent=OUT.so [--calls=200] [--hook-calls=2000]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pquic_amd import Engine  # noqa: E402
from span_model import SpanModel, pack  # noqa: E402  (what the repairs determine)


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith(f"--{name}=")), default)


calls, hook_calls, parent_path = int(arg("calls", 200)), int(arg("hook-calls", 2000)), arg("parent", None)
if not parent_path or not os.path.exists(parent_path):
    sys.exit("--parent=OUT.so: a build of the parent commit (tools/build_at_commit.sh) is the yardstick")
dev = torch.device("cuda:0")
this, parent = Engine(0), Engine(0, lib_path=parent_path)
assert not hasattr(parent.lib, "fecgpu_rlc_span_one_launch_calls"), "the parent build has the one-launch path"
variants = [("parent", parent, {}), ("this", this, {}), ("plan1", this, {"plan": 1})]
SHAPES = [("K30 R6", 30, [(0, 30, 6)]), ("K125 R20", 125, [(5 * o, 30, 1) for o in range(20)])]
L, P = 1200, 0.03
model = SpanModel()


def to_dev(a):
    a = np.ascontiguousarray(a)
    a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(a).to(dev)


def setup(K, windows, nb, seed):
    R = sum(w[2] for w in windows)
    rng = np.random.default_rng(seed)
    src = torch.from_numpy(rng.integers(0, 256, (nb, K, L), dtype=np.uint8)).to(dev)
    parts = []
    for o, n, r in windows:  # window (o, n, r) of every span: the spans' columns are one stream, K apart
        out = torch.empty((nb, r, L), dtype=torch.uint8, device=dev)
        this.rlc_window_encode(src.view(nb * K, L)[o:], out, nb, K, n, r, L)
        parts.append(out)
    rep = torch.cat(parts, dim=1).contiguous()
    seeds = np.tile(np.concatenate([np.arange(r) for _, _, r in windows]).astype(np.uint32), (nb, 1))
    off = np.tile(np.concatenate([np.full(r, o) for o, _, r in windows]).astype(np.uint8), (nb, 1))
    nss = np.tile(np.concatenate([np.full(r, n) for _, n, r in windows]).astype(np.uint8), (nb, 1))
    present, rpresent = rng.random((nb, K)) >= P, rng.random((nb, R)) >= P
    present[0, K // 2] = False  # the first span has a loss whatever the draw
    sp, rp = pack(present), pack(rpresent)
    s = model.solve(K, seeds, off, nss, sp, rp)
    work = src.clone()
    work[torch.from_numpy(~present).to(dev)] = 0xA5
    srow = work.data_ptr() + np.arange(nb * K, dtype=np.uint64) * L
    rrow = rep.data_ptr() + np.arange(nb * R, dtype=np.uint64) * L
    t = dict(K=K, R=R, nb=nb, src=src, work=work, rep=rep, s=s,
             args=[to_dev(x) for x in (srow, np.full(nb * K, L, np.uint32), rrow, np.full(nb * R, L, np.uint32),
                                       np.full(nb, L, np.uint32), seeds, off, nss, sp, rp)],
             st=torch.empty(nb, dtype=torch.uint8, device=dev), rec=torch.empty((nb, 2), dtype=torch.int64, device=dev),
             ws=this.alloc_workspace(nb, K, R))
    return t


def call(e, t):
    e.rlc_span_decode_rows_fused(*t["args"], t["st"], t["rec"], t["nb"], t["K"], t["R"], L, workspace=t["ws"])
    torch.cuda.current_stream().synchronize()


def set_knobs(e, kv):
    old = {k: e.get_knob(k) for k in kv}
    for k, v in kv.items():
        e.set_knob(k, v)
    return old


print(f"# span decode on rows, one call, host clock to the end of a synchronise; L {L}, p {P}, {calls} calls per cell, "
      "variants alternating", flush=True)
print(f"# {'shape':9s} {'spans':>5s} {'lost':>5s} {'det':>5s}  " +
      "  ".join(f"{n + ' med (min-max) us':>30s}" for n, _, _ in variants) + "   one-launch calls (this)", flush=True)
verdict = {}
for name, K, windows in SHAPES:
    for nb in (1, 8, 64):
        t = setup(K, windows, nb, [K, nb])
        ref = None
        for vname, e, kv in variants:  # equal outputs first (and the warm-up of every variant)
            old = set_knobs(e, kv)
            t["work"][torch.from_numpy(t["s"].miss).to(dev)] = 0xA5
            t["st"].fill_(0xEE)
            for _ in range(3):
                call(e, t)
            set_knobs(e, old)
            got = (t["st"].cpu().numpy().copy(), t["rec"].cpu().numpy().copy(), t["work"].cpu().numpy().copy())
            if ref is None:
                ref = got
                det = torch.from_numpy(t["s"].det).to(dev)
                assert np.array_equal(got[0], t["s"].status) and torch.equal(t["work"][det], t["src"][det])
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), f"{vname} differs from {variants[0][0]}"
        times = {v[0]: [] for v in variants}
        c0 = this.span_one_launch_calls()
        for _ in range(calls):
            for vname, e, kv in variants:
                old = set_knobs(e, kv)
                t0 = time.perf_counter()
                call(e, t)
                times[vname].append((time.perf_counter() - t0) * 1e6)
                set_knobs(e, old)
        one = this.span_one_launch_calls() - c0
        cells = [f"{statistics.median(times[n]):9.1f} ({min(times[n]):7.1f}-{max(times[n]):8.1f})" for n, _, _ in variants]
        print(f"  {name:9s} {nb:5d} {int(t['s'].miss.sum()):5d} {int(t['s'].det.sum()):5d}  " +
              "  ".join(f"{c:>30s}" for c in cells) + f"   {one}", flush=True)
        verdict[(name, nb)] = statistics.median(times["this"]) < min(times["parent"])
print("# decision rule: the one-launch path stays the default at a span count only if its median lies below the "
      "parent's min-max band there, for both shapes")
for nb in (1, 8, 64):
    print(f"#   {nb:2d} spans: " + ", ".join(f"{n} {'below' if verdict[(n, nb)] else 'NOT below'}" for n, _, _ in SHAPES) +
          f" -> {'holds' if all(verdict[(n, nb)] for n, _, _ in SHAPES) else 'does not hold'}")

# ---- the blocking hook call, one span per call
d = C.CDLL(os.path.join(ROOT, "tools", "libspanload.so"))
d.sl_run_blocking.argtypes = [C.c_int] * 6 + [C.c_double, C.c_long, C.c_int, C.c_uint, C.POINTER(C.c_double)]
print(f"# pquic_fec_rlc_recover_span, one span per call, losses redrawn per call (p {P}), {hook_calls} draws; the call "
      "to its return, host clock")
print(f"# {'shape':9s} {'arena':>10s} {'p50 us':>8s} {'p99 us':>8s} {'min us':>8s} {'lost':>6s} {'recovered':>9s} "
      f"{'in place':>9s} {'staged':>8s} {'errors':>6s} {'calls':>6s}")
for name, k, r, step, nwin in (("K30 R6", 30, 6, 30, 1), ("K125 R20", 30, 1, 5, 20)):
    for reg in (1, 0):
        out = (C.c_double * 9)()
        rc = d.sl_run_blocking(0, k, r, step, nwin, L, P, hook_calls, reg, 7, out)
        assert rc == 0, rc
        print(f"  {name:9s} {'registered' if reg else 'pageable':>10s} {out[0]:8.1f} {out[1]:8.1f} {out[2]:8.1f} "
              f"{int(out[3]):6d} {int(out[4]):9d} {int(out[5]):9d} {int(out[6]):8d} {int(out[7]):6d} {int(out[8]):6d}", flush=True)
