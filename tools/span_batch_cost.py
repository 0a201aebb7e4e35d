"""Span jobs of the batching adapter under load (tools/libspanload.so, sl_run): 64 connections with registered
arenas submit spans made of k / r / step windows under independent loss; span_compact 0 against 1, interleaved
runs in one process.  Per shape and loss: spans/s, recovered symbols/s, the share of lost symbols recovered,
stream GiB/s (received bytes handed over) and the p50 / p99 submit-to-completion latency -- medians with
min-max over the runs.
usage: python tools/span_batch_cost.py [--runs N] [--spans N] [--conn N] [--batch N]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--spans", type=int, default=16384)
ap.add_argument("--conn", type=int, default=64)
ap.add_argument("--slots", type=int, default=8, help="spans a connection keeps in flight at most")
ap.add_argument("--batch", type=int, default=256, help="batch_blocks of the batcher")
ap.add_argument("--delay", type=int, default=2000, help="max_delay_us")
args = ap.parse_args()

eng = C.CDLL(os.path.join(ROOT, "pquic_amd", "lib", "libpquic_fec.so"))
eng.fecgpu_set_knob.argtypes = [C.c_char_p, C.c_int]
drv = C.CDLL(os.path.join(ROOT, "tools", "libspanload.so"))
drv.sl_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_long, C.c_int,
                       C.c_uint, C.c_uint, C.c_int, C.c_uint, C.POINTER(C.c_double)]


def med(xs):
    return f"{statistics.median(xs):10.1f} ({min(xs):.1f} - {max(xs):.1f})"


def leg(k, r, step, p):
    nwin = min((128 - k) // step + 1, 128 // r)
    res = {0: [], 1: []}
    for run in range(args.runs + 1):  # run 0 warms up (page-locking, first launches) and is dropped
        for knob in (0, 1):
            assert eng.fecgpu_set_knob(b"span_compact", knob) == 0
            out = (C.c_double * 12)()
            rc = drv.sl_run(0, args.conn, k, r, step, nwin, 1200, p, args.spans, args.slots, args.batch, args.delay, 1,
                            7 + run, out)
            assert rc == 0 and out[10] == 0, (rc, list(out))
            if run:
                res[knob].append(list(out))
    eng.fecgpu_set_knob(b"span_compact", 1)
    K, R = k + (nwin - 1) * step, nwin * r
    print(f"k{k} r{r} step {step}: K {K}, R {R}, L 1200, loss {p:g}, {args.conn} connections x {args.slots} spans in "
          f"flight, {args.spans} spans per run, batch_blocks {args.batch}, max_delay {args.delay} us, {args.runs} runs")
    for knob in (0, 1):
        rows = res[knob]
        col = lambda i: [x[i] for x in rows]  # noqa: E731
        share = [100 * x[6] / max(x[5], 1) for x in rows]
        print(f"  span_compact {knob}: spans/s {med(col(0))}  recovered symbols/s {med(col(1))}  recovered "
              f"{statistics.median(share):.2f} % of lost  stream GiB/s {med(col(2))}  p50 us {med(col(3))}  "
              f"p99 us {med(col(4))}  rows staged {int(max(col(8)))}  batches {int(statistics.median(col(9)))}",
              flush=True)


for shape in ((30, 1, 5), (32, 8, 8)):
    for p in (0.01, 0.03):
        leg(*shape, p)
