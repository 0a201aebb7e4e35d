"""What window jobs in place cost or save (profiles/window_rows.log).
load: the window sender of tools/batch_load.c (bl_run_window_rows) with the symbols in a registered arena
  (the batcher hands rows over where they lie) and with the arena left unregistered (every row staged, the
  path of before), 64 connections, equal 1200-byte symbols under a 1200-byte batcher and ragged symbols
  (bl_set_ragged) under a 1500-byte batcher; one line per run, runs of the two settings alternating.
  Against a library built from another commit (LD_LIBRARY_PATH or a libbatchload.so linked to it) the same
  command measures that commit: there registering changes nothing.
dev: on device-resident rows, fecgpu_rlc_window_encode_rows against rows_gather +
  fecgpu_rlc_window_encode_table + rows_scatter (the three-pass equivalent), 2^16 windows of k32 r8 step 8,
  equal 1200-byte rows and ragged ones; medians and ranges of the events' times.
usage (GPU box): python tools/window_rows_cost.py load [TAG] [runs] [batch] [windows] [libbatchload.so]
                 python tools/window_rows_cost.py dev [cycles]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(30, 1, 5), (30, 5, 25)]  # the bench's two window shapes: k, r, step


def load(tag, runs, batch, nwin, path):
    lib = C.CDLL(path)
    lib.bl_run_window_rows.argtypes = [C.c_int] * 6 + [C.c_long, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                       C.POINTER(C.c_double)]
    lib.bl_set_ragged.argtypes = [C.c_int, C.c_uint]
    lib.bl_last_rows.argtypes = [C.POINTER(C.c_double)]
    for run in range(runs):
        for ragged in (0, 1):
            lib.bl_set_ragged(1500 if ragged else 0, 7)
            for k, r, step in SHAPES:
                for reg in (1, 0):
                    out, rows = (C.c_double * 8)(), (C.c_double * 2)()
                    rc = lib.bl_run_window_rows(0, k, r, 1200, step, 64, nwin, batch, 2000, 2, reg, out)
                    lib.bl_last_rows(rows)
                    print(f"{tag} run {run} {'ragged' if ragged else 'equal '} k{k} r{r} step {step:2d} "
                          f"{'registered  ' if reg else 'unregistered'}: rc {rc} stream {out[0]:6.2f} GiB/s "
                          f"p50 {out[1]:6.0f} us p99 {out[2]:6.0f} us batches {int(out[4])} "
                          f"in_place {int(rows[0])} staged {int(rows[1])}", flush=True)


def dev(cycles):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pquic_amd import Engine
    eng = Engine(0)
    d = torch.device("cuda:0")
    k, r, step, L, nwin = 32, 8, 8, 1200, 1 << 16
    nrows = (nwin - 1) * step + k
    rng = np.random.default_rng(1)
    src = torch.empty((nrows, L), dtype=torch.uint8, device=d)
    eng.synth_fill(src, src.numel(), 3, 0)
    rep = torch.zeros((nwin * r, L), dtype=torch.uint8, device=d)
    rows = torch.from_numpy((src.data_ptr() + np.arange(nrows, dtype=np.int64) * L)).to(d)
    reps = torch.from_numpy((rep.data_ptr() + np.arange(nwin * r, dtype=np.int64) * L)).to(d)
    wrow = torch.from_numpy((np.arange(nwin, dtype=np.int64) * step).astype(np.int32)).to(d)
    ws = torch.empty(eng.window_rows_workspace_bytes(nrows, L), dtype=torch.uint8, device=d)
    packed = torch.empty((nwin * r, L), dtype=torch.uint8, device=d)
    for name in ("equal", "ragged"):
        if name == "equal":
            ln = np.full(nrows, L, np.int32)
        else:  # half full, a quarter in [L/2, L], a quarter in [40, L/2]: the ragged legs' mix
            kind = rng.integers(0, 4, nrows)
            ln = np.where(kind < 2, L, np.where(kind == 2, rng.integers(L // 2, L + 1, nrows),
                                                rng.integers(40, L // 2 + 1, nrows))).astype(np.int32)
        blk = np.array([ln[w * step: w * step + k].max() for w in range(nwin)], np.int32)
        row_len, blk_len = torch.from_numpy(ln).to(d), torch.from_numpy(blk).to(d)
        rep_len = torch.from_numpy(np.repeat(blk, r)).to(d)

        def one():
            eng.rlc_window_encode_rows(rows, row_len, nrows, wrow, reps, blk_len, nwin, k, r, L, workspace=ws)

        def three():
            eng.rows_gather(rows, row_len, nrows, L, ws)
            eng.rlc_window_encode_table(ws, nrows, wrow, packed, nwin, k, r, L)
            eng.rows_scatter(packed, reps, rep_len, nwin * r, L)
        one()
        torch.cuda.synchronize()
        a = rep.clone()
        rep.zero_()
        three()
        torch.cuda.synchronize()
        same = bool(torch.equal(a, rep))
        times = {"fused_rows": [], "gather_table_scatter": []}
        for _ in range(cycles):
            for tag, fn in (("fused_rows", one), ("gather_table_scatter", three)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[tag].append(e0.elapsed_time(e1))
        for tag, t in times.items():
            print(f"dev {name} k{k} r{r} step {step} 2^16 windows {tag:<21}: median {statistics.median(t):7.3f} ms "
                  f"min {min(t):7.3f} max {max(t):7.3f} (n {len(t)}) same bytes {same}", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "dev":
        dev(int(a[1]) if len(a) > 1 else 15)
    else:
        load(a[1] if len(a) > 1 else "tree", int(a[2]) if len(a) > 2 else 3, int(a[3]) if len(a) > 3 else 1536,
             int(a[4]) if len(a) > 4 else 100000,
             a[5] if len(a) > 5 else os.path.join(ROOT, "tools", "libbatchload.so"))
