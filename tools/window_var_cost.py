"""What windows of their own length in one call and one job cost or save (profiles/window_var.log).
dev: fecgpu_rlc_window_encode_rows_var_host on device-resident rows, 2^16 windows of 1200-byte symbols, r 1 and
  r 5, the windows' ends two symbols apart, lengths (a) a random walk in 1..30 by steps of -3..+3, (b) uniform in
  1..30, (c) all 30 -- against what the parent commit can do with the same rows, built from existing entry
  points in the same process: one fecgpu_rlc_window_encode_rows_host call per distinct length (`per-length`),
  and one fecgpu_rlc_encode_rows_fused_host call on blocks of 30 rows, the positions past a window's length
  rows of 0 bytes at address 0 (`padded`); for (c) also the plain rows form, which the call must be.  All
  variants alternate in one process on the same buffers, their tables page-locked; every time is a host clock
  around a call that returns after its streams have drained; medians with min-max over the repeats.
  THE RULE, stated before measuring: the sorted-class kernel stays the path for mixed lengths if its median for
  (a) and for (b) lies below the min-max band of both baselines.  Where it does not, the host form takes the
  faster baseline for that case.  The tool prints the verdict per case.
load: the window sender of tools/batch_load.c with bl_set_window_walk (every connection's window length a random
  walk in 1..30, min(r, length) repairs), 64 connections with the arena registered, batches of 1536, mixed jobs
  off against on (PQUIC_FEC_BATCH_WINDOW_MIXED, read when the batcher is created), runs alternating; then the
  constant-length load k30 r5 step 25 once with mixed jobs on.
usage (GPU box): python tools/window_var_cost.py dev [repeats]
                 python tools/window_var_cost.py load [runs] [batch] [windows] [libbatchload.so]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "PQUIC_FEC_BATCH_WINDOW_MIXED"


def load(runs, batch, nwin, path):
    lib = C.CDLL(path)
    lib.bl_run_window_rows.argtypes = [C.c_int] * 6 + [C.c_long, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                       C.POINTER(C.c_double)]
    lib.bl_set_window_walk.argtypes = [C.c_int, C.c_uint]
    lib.bl_last_rows.argtypes = [C.POINTER(C.c_double)]

    def one(tag, k, r, step, mixed):
        os.environ.pop(ENV, None)
        if mixed:
            os.environ[ENV] = "1"
        out, rows = (C.c_double * 8)(), (C.c_double * 2)()
        rc = lib.bl_run_window_rows(0, k, r, 1200, step, 64, nwin, batch, 2000, 2, 1, out)
        os.environ.pop(ENV, None)
        lib.bl_last_rows(rows)
        print(f"{tag} k{k} r{r} step {step:2d} mixed {'on ' if mixed else 'off'}: rc {rc} stream {out[0]:6.2f} GiB/s "
              f"windows {out[7]:6.2f} GiB/s p50 {out[1]:6.0f} us p99 {out[2]:6.0f} us batches {int(out[4])} "
              f"in_place {int(rows[0])} staged {int(rows[1])}", flush=True)
        return out[0], out[1], out[2]
    res = {0: [], 1: []}
    lib.bl_set_window_walk(1, 7)
    for run in range(runs):
        for mixed in (0, 1):
            for r, step in ((1, 5), (5, 25)):
                res[mixed].append(((r, step),) + one(f"walk run {run}", 30, r, step, mixed))
    for r, step in ((1, 5), (5, 25)):
        for mixed in (0, 1):
            for i, what in ((1, "stream GiB/s"), (2, "p50 us"), (3, "p99 us")):
                v = [x[i] for x in res[mixed] if x[0] == (r, step)]
                print(f"walk k<=30 r{r} step {step:2d} mixed {'on ' if mixed else 'off'} {what:12s}: median "
                      f"{statistics.median(v):8.2f} range {min(v):8.2f} .. {max(v):8.2f} ({len(v)} runs)")
    lib.bl_set_window_walk(0, 0)
    for mixed in (0, 1, 0, 1):
        one("constant", 30, 5, 25, mixed)


def dev(repeats):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pquic_amd import Engine
    from pquic_amd.engine import HostPath
    eng = Engine(0)
    lib = eng.lib
    lib.fecgpu_host_alloc.restype = C.c_void_p
    lib.fecgpu_host_alloc.argtypes = [C.c_size_t]
    hp = HostPath(0, nstreams=3)
    d = torch.device("cuda:0")
    kmax, L, nwin, step = 30, 1200, 1 << 16, 2

    def pinned(a):
        a = np.ascontiguousarray(a)
        p = lib.fecgpu_host_alloc(max(a.nbytes, 16))
        assert p
        out = np.frombuffer((C.c_uint8 * max(a.nbytes, 16)).from_address(p), np.uint8)[:a.nbytes].view(a.dtype)
        out = out.reshape(a.shape)
        out[...] = a
        return out
    nrows = (nwin - 1) * step + kmax
    src = torch.empty((nrows, L), dtype=torch.uint8, device=d)
    eng.synth_fill(src, src.numel(), 3, 0)
    rng = np.random.default_rng(11)
    end = kmax + step * np.arange(nwin, dtype=np.int64)
    walk = np.empty(nwin, np.int64)
    cur = 15
    for w, s in enumerate(rng.integers(-3, 4, nwin)):
        cur = min(max(cur + int(s), 1), kmax)
        walk[w] = cur
    cases = {"a walk": walk, "b uniform": rng.integers(1, kmax + 1, nwin), "c all 30": np.full(nwin, kmax)}
    rows = pinned(src.data_ptr() + np.arange(nrows, dtype=np.uint64) * L)
    row_len = pinned(np.full(nrows, L, np.uint32))
    blk_len = pinned(np.full(nwin, L, np.uint32))
    print(f"# {nwin} windows, L {L}, ends {step} symbols apart, {nrows} stream rows, {repeats} repeats, alternating")
    print("# rule: var stays the path for mixed lengths if its median for (a) and (b) is below both baselines' minimum")
    for r in (1, 5):
        rep = torch.zeros((nwin * r, L), dtype=torch.uint8, device=d)
        rep_rows = pinned(rep.data_ptr() + np.arange(nwin * r, dtype=np.uint64) * L)
        for name, wl in cases.items():
            wlen = pinned(wl.astype(np.uint8))
            wrow = pinned((end - wl).astype(np.uint32))
            # per-length: the windows of each length, their tables cut out beforehand
            per = []
            for x in np.unique(wl):
                idx = np.flatnonzero(wl == x)
                rr = (idx[:, None] * r + np.arange(r)[None, :]).ravel()
                per.append((int(x), len(idx), pinned(wrow[idx]), pinned(rep_rows[rr]), pinned(blk_len[idx])))
            # padded: blocks of kmax rows, the positions past the length rows of 0 bytes at address 0
            j = np.arange(kmax)[None, :]
            live = j < wl[:, None]
            pos = np.minimum(wrow.astype(np.int64)[:, None] + j, nrows - 1)
            prow = pinned(np.where(live, rows[pos], np.uint64(0)).astype(np.uint64))
            plen = pinned(np.where(live, L, 0).astype(np.uint32))
            pfbn = pinned(np.zeros(nwin, np.uint32))

            def var():
                hp.rlc_window_encode_rows_var(rows, row_len, nrows, wrow, wlen, rep_rows, blk_len, nwin, kmax, r, L)

            def per_length():
                for x, n, wr, rrw, bl in per:
                    hp.rlc_window_encode_rows(rows, row_len, nrows, wr, rrw, bl, n, x, r, L)

            def padded():
                hp.rlc_encode_rows_fused(prow, plen, rep_rows, blk_len, nwin, kmax, r, L, fbn=pfbn)

            def plain():
                hp.rlc_window_encode_rows(rows, row_len, nrows, wrow, rep_rows, blk_len, nwin, kmax, r, L)
            variants = [("var", var), ("per-length", per_length), ("padded", padded)]
            if name.startswith("c"):
                variants.append(("plain rows", plain))
            sums = {}
            for n, f in variants:  # the same bytes from every variant, and the warm-up
                rep.zero_()
                f()
                torch.cuda.synchronize()
                sums[n] = int(rep.view(torch.int64).sum().item())
            assert len(set(sums.values())) == 1, sums
            t = {n: [] for n, _ in variants}
            for _ in range(repeats):
                for n, f in variants:
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    t[n].append((time.perf_counter() - t0) * 1e3)
            for n, _ in variants:
                print(f"r{r} ({name:9s}) {n:10s}: median {statistics.median(t[n]):7.3f} ms  range {min(t[n]):7.3f} .. "
                      f"{max(t[n]):7.3f}  ({len(np.unique(wl))} lengths)", flush=True)
            if not name.startswith("c"):
                med = statistics.median(t["var"])
                ok = med < min(t["per-length"]) and med < min(t["padded"])
                best = min(("per-length", "padded"), key=lambda n: statistics.median(t[n]))
                print(f"r{r} ({name:9s}) verdict: var median {'below' if ok else 'NOT below'} both baselines' bands"
                      f"{'' if ok else ' -> the faster baseline is ' + best}", flush=True)
    hp.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "dev":
        dev(int(a[1]) if len(a) > 1 else 30)
    elif a and a[0] == "load":
        load(int(a[1]) if len(a) > 1 else 9, int(a[2]) if len(a) > 2 else 1536, int(a[3]) if len(a) > 3 else 400000,
             a[4] if len(a) > 4 else os.path.join(ROOT, "tools", "libbatchload.so"))
    else:
        print(__doc__)
