"""What full-rank decode costs next to reference-mode decode: both modes in one process on the same
device buffers, interleaved, staged (plan | packed apply) and timed with events.

Workloads: k16 r4 e4 L1200, 2^20 blocks (the bench's seeded 4-subsets) and k64 r16 e16 L9000, 2^16
blocks; every repair received.  Per mode and stage: median and min-max over the repeats; the share of
blocks only full mode recovers.  The bar is set by the reference-mode figures of the same run: full
mode's median total may exceed reference mode's by that share (the extra blocks' rows are real
traffic) plus reference mode's own min-max spread.
usage: python tools/full_decode_cost.py [--repeats N] [--small]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pquic_amd import BLOCK_RECOVERED, BLOCK_REF_UB, BLOCK_SINGULAR, Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--small", action="store_true", help="1/16 of the blocks (a quick look, not the committed figures)")
args = ap.parse_args()
assert args.repeats >= 20, "at least 20 repeats per mode"

eng = Engine(0)
dev = torch.device("cuda:0")


def make_erasures(nb, k, e, seed):
    """bench.py's erasure patterns: e distinct random source erasures per block, masks [nb, 2] int64."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    keys = torch.rand((nb, k), generator=g)
    miss = keys.argsort(dim=1)[:, :e]
    pres = torch.ones((nb, 128), dtype=torch.bool)
    pres[:, k:] = False
    pres.scatter_(1, miss, False)
    sp = torch.zeros((nb, 2), dtype=torch.int64)
    for w in range(2):
        bits = pres[:, 64 * w: 64 * w + 64].to(torch.int64)
        lo = (bits[:, :63] << torch.arange(63, dtype=torch.int64)).sum(1)
        sp[:, w] = lo | (bits[:, 63] << 63)
    return sp.to(dev), miss.sort(dim=1).values.to(dev)


def med_range(xs):
    return f"{statistics.median(xs):10.1f} us  ({min(xs):.1f} - {max(xs):.1f})"


def workload(k, r, e, L, nb):
    src = torch.empty((nb, k, L), dtype=torch.uint8, device=dev)
    eng.synth_fill(src, src.numel(), 0x5EEDF3C0, 0)
    rep = torch.empty((nb, r, L), dtype=torch.uint8, device=dev)
    eng.rlc_encode(src, rep, k, r, L, nblocks=nb)
    sp, miss = make_erasures(nb, k, e, 11)
    rp = torch.zeros((nb, 2), dtype=torch.int64, device=dev)
    rp[:, 0] = (1 << r) - 1
    work = src.clone()
    work.view(nb * k, L)[(torch.arange(nb, device=dev).unsqueeze(1) * k + miss).reshape(-1)] = 0xA5
    dst = torch.empty((nb, min(k, r), L), dtype=torch.uint8, device=dev)
    ws = eng.alloc_workspace(nb, k, r)
    out = {m: (torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty((nb, 2), dtype=torch.int64, device=dev))
           for m in ("ref", "full")}
    plan = {"ref": lambda: eng.rlc_decode_plan(sp, rp, k, r, nb, ws),
            "full": lambda: eng.rlc_decode_plan_full(sp, rp, k, r, nb, ws)}

    def once(mode, ev=None):
        st, rec = out[mode]
        if ev:
            ev[0].record()
        plan[mode]()
        if ev:
            ev[1].record()
        eng.rlc_decode_apply_packed(work, rep, dst, st, rec, k, r, L, nb, ws)
        if ev:
            ev[2].record()

    for _ in range(3):  # warm-up, both modes
        once("ref")
        once("full")
    torch.cuda.synchronize()
    t = {m: {"plan": [], "apply": [], "total": []} for m in ("ref", "full")}
    for _ in range(args.repeats):  # interleaved: drift hits both modes alike
        for mode in ("ref", "full"):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            once(mode, ev)
            ev[2].synchronize()
            t[mode]["plan"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            t[mode]["apply"].append(ev[1].elapsed_time(ev[2]) * 1e3)
            t[mode]["total"].append(ev[0].elapsed_time(ev[2]) * 1e3)
    # what each mode recovered (the last full-mode run's rows are in dst: check them against the sources)
    st_r, st_f = out["ref"][0], out["full"][0]
    n_ref = int((st_r == BLOCK_RECOVERED).sum())
    n_full = int((st_f == BLOCK_RECOVERED).sum())
    assert int((st_f == BLOCK_REF_UB).sum()) == 0 and bool((st_f[st_r == BLOCK_RECOVERED] == BLOCK_RECOVERED).all())
    okb = (st_f == BLOCK_RECOVERED).nonzero().squeeze(1)
    for c0 in range(0, okb.numel(), 1 << 14):
        b = okb[c0:c0 + (1 << 14)]
        assert bool((dst[b, :e] == src.view(nb, k, L)[b.unsqueeze(1), miss[b]]).all()), "recovered rows differ"
    extra = (n_full - n_ref) / n_ref
    print(f"k{k} r{r} e{e} L{L}, {nb} blocks, {args.repeats} interleaved repeats per mode")
    print(f"  recovered: reference mode {n_ref}, full mode {n_full} (+{n_full - n_ref} blocks, +{100 * extra:.2f} %), "
          f"singular {int((st_f == BLOCK_SINGULAR).sum())}; full-mode rows equal the sources")
    for mode in ("ref", "full"):
        for stage in ("plan", "apply", "total"):
            print(f"  {mode:4s} {stage:5s} {med_range(t[mode][stage])}")
    ref_med, full_med = statistics.median(t["ref"]["total"]), statistics.median(t["full"]["total"])
    spread = max(t["ref"]["total"]) - min(t["ref"]["total"])
    bar = ref_med * (1 + extra) + spread
    verdict = "within the bar" if full_med <= bar else f"OVER the bar by {full_med - bar:.1f} us"
    print(f"  full - ref median total {full_med - ref_med:+.1f} us ({100 * (full_med / ref_med - 1):+.2f} %); "
          f"bar {bar:.1f} us = ref {ref_med:.1f} x (1 + {extra:.4f}) + ref spread {spread:.1f}: {verdict}", flush=True)


div = 16 if args.small else 1
workload(16, 4, 4, 1200, (1 << 20) // div)
torch.cuda.empty_cache()
workload(64, 16, 16, 9000, (1 << 16) // div)
