"""What the joint decode of overlapping windows recovers that window-by-window decoding does not (CPU, on the
numpy model tests/span_model.py; no device).

For the window shapes bench.py uses -- k30 r1 step 5, k30 r5 step 25, k32 r8 step 8 -- a span holds as many
whole windows as 128 columns and 128 repair slots allow.  Sources and repairs are lost independently with
probability p.  Reported: the share of lost source symbols recovered
  alone      each window decoded by itself in full-rank mode from the received symbols (fecgpu_rlc_decode_full),
  chained    the same, a recovered symbol counting as received by the windows after it, until nothing changes,
  jointly    by the span decode.
The first and last columns of a span lie in fewer of its windows than a stream's interior symbols do, so all
three shares understate a long stream alike.
usage: python tools/span_recovery_gain.py [--spans N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

from span_model import SpanModel, pack  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spans", type=int, default=20000)
args = ap.parse_args()

model = SpanModel()
CHUNK = 2000
print(f"{args.spans} spans per row; seeds: sources and repairs lost independently, numpy default_rng([k, r, step, 1000 p])")
print(f"{'shape':18s} {'K':>4s} {'R':>4s} {'p':>5s} {'lost':>8s} {'alone':>8s} {'chained':>8s} {'jointly':>8s}")
for k, r, step in ((30, 1, 5), (30, 5, 25), (32, 8, 8)):
    W = min((128 - k) // step + 1, 128 // r)
    K, R = k + (W - 1) * step, W * r
    seed = np.tile(np.tile(np.arange(r), W).astype(np.uint32), (CHUNK, 1))  # window blocks carry block number 0
    off = np.tile(np.repeat(np.arange(W) * step, r).astype(np.uint8), (CHUNK, 1))
    nss = np.full((CHUNK, R), k, np.uint8)
    for p in (0.01, 0.03, 0.10):
        rng = np.random.default_rng([k, r, step, int(1000 * p)])
        lost = alone = chained = joint = 0
        t0 = time.time()
        for c0 in range(0, args.spans, CHUNK):
            n = min(CHUNK, args.spans - c0)
            present = rng.random((n, K)) >= p
            rpresent = rng.random((n, R)) >= p
            s = model.solve(K, seed[:n], off[:n], nss[:n], pack(present), pack(rpresent))
            a = model.windows_alone(s, off[:n], nss[:n])
            c = model.windows_alone(s, off[:n], nss[:n], propagate=True)
            assert not (a & ~c).any() and not (c & ~s.det).any()  # each recovers what the one before it does
            lost += int(s.miss.sum())
            alone += int(a.sum())
            chained += int(c.sum())
            joint += int(s.det.sum())
        print(f"k{k} r{r} step {step:<6d} {K:4d} {R:4d} {p:5.2f} {lost:8d} {100 * alone / lost:7.2f}% "
              f"{100 * chained / lost:7.2f}% {100 * joint / lost:7.2f}%   ({time.time() - t0:.0f} s)", flush=True)
