"""What ragged rows cost and save: the figures of profiles/ragged_rows.log.

  device   fecgpu_rlc_encode_rows_len / fecgpu_rlc_decode_rows_len with every length equal to symbol_size
           against fecgpu_rlc_encode_rows / fecgpu_rlc_decode_rows on the same device-resident rows: k16 r4
           L1200 at 2^16 blocks and k64 r16 L9000 at 2^12 blocks, interleaved, timed with events.  The
           _len forms move every row through device memory twice more (gather, scatter): the ratio is
           their price, recorded so nobody calls them free.  The one-pass forms (fecgpu_rlc_*_rows_fused) run
           beside them, and a second pass repeats all six on ragged rows (the lengths of `copies`, the block
           as long as its longest source): the figures of profiles/rows_fused.log.
  copies   the gather and scatter kernels alone on the k16 r4 L1200 rows (device memory and page-locked
           host memory): the A/B behind their launch shape, one line per library build
           (PQUIC_AMD_LIB selects a build with another -DFEC_ROWS_LPR).
  load     ONE run of each batcher leg through tools/libbatchload.so (or --loadlib: the same generator
           linked against another tree's engine): ragged generate and recover (max_symbol 1500, block
           length 1200, 64 connections with registered arenas) and the equal-length generate and recover
           legs of bench.py's batch_saturated.  Prints one JSON line; run it alternately per tree.
  summary  medians and quartiles of the JSON lines of two trees (files given as --a / --b).
usage: python tools/ragged_rows_cost.py device|copies|load|summary [options]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["device", "copies", "load", "summary"])
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--loadlib", default=os.path.join(ROOT, "tools", "libbatchload.so"))
ap.add_argument("--tag", default="head")
ap.add_argument("--blocks", type=int, default=200000)
ap.add_argument("--a")
ap.add_argument("--b")
args = ap.parse_args()


def med_range(xs):
    return f"{statistics.median(xs):9.1f} us ({min(xs):.1f} - {max(xs):.1f})"


def timed(fns, repeats):
    """Interleaved event timings (us) of the callables in fns: {name: [..]}"""
    import torch
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {n: [] for n in fns}
    for _ in range(repeats):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[n].append(e0.elapsed_time(e1) * 1e3)
    return t


def device_rows(eng, torch, k, r, L, nb, e):
    """Device-resident rows with their tables: sources, repairs (encoded), e erasures per block."""
    dev = torch.device("cuda:0")
    src = torch.empty((nb, k, L), dtype=torch.uint8, device=dev)
    eng.synth_fill(src, src.numel(), 0x5EEDF3C0, 0)
    rep = torch.empty((nb, r, L), dtype=torch.uint8, device=dev)
    srow = src.data_ptr() + torch.arange(nb * k, dtype=torch.int64, device=dev) * L
    rrow = rep.data_ptr() + torch.arange(nb * r, dtype=torch.int64, device=dev) * L
    slen = torch.full((nb * k,), L, dtype=torch.int32, device=dev)
    rlen = torch.full((nb * r,), L, dtype=torch.int32, device=dev)
    blen = torch.full((nb,), L, dtype=torch.int32, device=dev)
    return src, rep, srow, rrow, slen, rlen, blen


def mode_device():
    import torch
    from pquic_amd import Engine
    eng = Engine(0)
    dev = torch.device("cuda:0")
    for k, r, L, nb, e in ((16, 4, 1200, 1 << 16, 4), (64, 16, 9000, 1 << 12, 16)):
        src, rep, srow, rrow, slen, rlen, blen = device_rows(eng, torch, k, r, L, nb, e)
        ws = eng.alloc_rows_len_workspace(nb, k, r, L)
        dws = eng.alloc_workspace(nb, k, r)
        eng.rlc_encode_rows(srow, rrow, nb, k, r, L)
        torch.cuda.synchronize()
        keep = rep.clone()
        seeds = ((torch.arange(nb, dtype=torch.int64, device=dev).unsqueeze(1) << 8) |
                 torch.arange(r, dtype=torch.int64, device=dev)).to(torch.int32).reshape(-1)
        sp = torch.zeros((nb, 2), dtype=torch.int64, device=dev)
        lost = torch.arange(nb, device=dev) % (k - e + 1)  # sources lost .. lost + e - 1, as the load generator
        full = (1 << k) - 1 if k < 64 else -1
        if k < 64:
            sp[:, 0] = full & ~(((1 << e) - 1) << lost)
        else:
            sp[:, 0] = ~(((1 << e) - 1) << lost)
        rp = torch.zeros((nb, 2), dtype=torch.int64, device=dev)
        rp[:, 0] = (1 << r) - 1
        st = torch.empty(nb, dtype=torch.uint8, device=dev)
        rec = torch.empty((nb, 2), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def dec_rows():
            rc = eng.lib.fecgpu_rlc_decode_rows(srow.data_ptr(), rrow.data_ptr(), nb, k, r, L, seeds.data_ptr(),
                                                sp.data_ptr(), rp.data_ptr(), st.data_ptr(), rec.data_ptr(),
                                                dws.data_ptr(), dws.numel(), stream)
            assert rc == 0, eng.err()

        fused = hasattr(eng.lib, "fecgpu_rlc_encode_rows_fused")  # an older build (PQUIC_AMD_LIB) lacks the legs
        rag_s = torch.randint(40, L + 1, (nb * k,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(dev)
        rag_b = rag_s.reshape(nb, k).max(1).values.contiguous()
        rag_r = rag_b.repeat_interleave(r).contiguous()
        for what, sl, rl, bl in (("equal lengths", slen, rlen, blen), ("ragged lengths", rag_s, rag_r, rag_b)):
            fns = {
                "encode_rows": lambda: eng.rlc_encode_rows(srow, rrow, nb, k, r, L),
                "encode_rows_len": lambda: eng.rlc_encode_rows_len(srow, sl, rrow, bl, nb, k, r, L, workspace=ws),
                "decode_rows": dec_rows,
                "decode_rows_len": lambda: eng.rlc_decode_rows_len(srow, sl, rrow, rl, bl, seeds, sp, rp, st, rec,
                                                                  nb, k, r, L, workspace=ws),
            }
            if fused:
                fns["encode_rows_fused"] = lambda: eng.rlc_encode_rows_fused(srow, sl, rrow, bl, nb, k, r, L)
                fns["decode_rows_fused"] = lambda: eng.rlc_decode_rows_fused(srow, sl, rrow, rl, bl, seeds, sp, rp, st,
                                                                            rec, nb, k, r, L, workspace=dws)
            if sl is slen:
                for n in ("encode_rows_len", "encode_rows_fused") if fused else ("encode_rows_len",):
                    rep.zero_()
                    fns[n]()
                    torch.cuda.synchronize()
                    assert torch.equal(rep, keep), f"{n} differs from encode_rows"
            t = timed(fns, args.repeats)
            payload = int(sl.sum())
            print(f"k{k} r{r} e{e} L{L}, {nb} blocks, device-resident rows, {what}, {args.repeats} interleaved repeats")
            for n, xs in t.items():
                print(f"  {n:18s} {med_range(xs)}  {payload / statistics.median(xs) / 1073.741824:8.1f} GiB/s payload")
            for a, b in (("encode_rows_len", "encode_rows"), ("decode_rows_len", "decode_rows")):
                print(f"  {a} / {b}: x{statistics.median(t[a]) / statistics.median(t[b]):.2f}", flush=True)
            if fused:
                for a in ("encode", "decode"):
                    f, ln, eq = t[a + "_rows_fused"], t[a + "_rows_len"], t[a + "_rows"]
                    print(f"  {a}_rows_fused / {a}_rows: x{statistics.median(f) / statistics.median(eq):.2f}; "
                          f"fused median {statistics.median(f):.1f} us against the minimum of {a}_rows_len "
                          f"{min(ln):.1f} us: {'below' if statistics.median(f) < min(ln) else 'NOT below'}", flush=True)
        del src, rep, ws, dws, keep
        torch.cuda.empty_cache()


def mode_copies():
    import torch
    from pquic_amd import Engine
    from pquic_amd.engine import LIB_PATH
    eng = Engine(0)
    dev = torch.device("cuda:0")
    k, r, L, nb = 16, 4, 1200, 1 << 16
    n = nb * k
    eng.lib.fecgpu_host_alloc.restype = C.c_void_p
    eng.lib.fecgpu_host_alloc.argtypes = [C.c_size_t]
    eng.lib.fecgpu_host_free.argtypes = [C.c_void_p]
    packed = torch.empty((n, L), dtype=torch.uint8, device=dev)
    eng.synth_fill(packed, packed.numel(), 1, 0)
    rows_d = torch.empty((n, L), dtype=torch.uint8, device=dev)
    host = eng.lib.fecgpu_host_alloc(n * L)
    assert host
    d = C.c_uint64(0)
    assert eng.lib.fecgpu_host_device_address(host, n * L, C.byref(d)) == 0
    idx = torch.arange(n, dtype=torch.int64, device=dev) * L
    lens = {"equal": torch.full((n,), L, dtype=torch.int32, device=dev),
            "ragged": (torch.randint(40, L + 1, (n,), generator=torch.Generator().manual_seed(7))
                       .to(torch.int32).to(dev))}
    print(f"library {os.path.relpath(LIB_PATH, ROOT)}: gather / scatter of {n} rows of {L} B")
    for where, base in (("device rows", rows_d.data_ptr()), ("page-locked host rows", d.value)):
        tab = base + idx
        for ln, lv in lens.items():
            t = timed({"gather": lambda: eng.rows_gather(tab, lv, n, L, packed),
                       "scatter": lambda: eng.rows_scatter(packed, tab, lv, n, L)}, args.repeats)
            moved = int(lv.sum())
            for name, xs in t.items():
                print(f"  {where:22s} {ln:6s} {name:7s} {med_range(xs)}  "
                      f"{moved / statistics.median(xs) / 1073.741824:7.1f} GiB/s", flush=True)
    eng.lib.fecgpu_host_free(host)


def mode_load():
    lib = C.CDLL(args.loadlib)
    D = C.POINTER(C.c_double)
    lib.bl_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_uint, C.c_uint, C.c_int,
                           C.c_double, C.c_int, D]
    lib.bl_run_recover.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_uint,
                                   C.c_uint, C.c_int, C.c_int, D]
    lib.bl_set_inflight.argtypes = [C.c_int]
    lib.bl_set_ragged.argtypes = [C.c_int, C.c_uint]
    for f in ("bl_last_rows", "bl_last_phases", "bl_last_latency"):
        getattr(lib, f).argtypes = [D]
    REG, PER_CONN = 1, 2
    k, r, L, e, nconn, batch = 16, 4, 1200, 4, 64, 2048  # bench.py's batch_saturated legs
    lib.bl_set_inflight(3)
    warm = (C.c_double * 8)()
    lib.bl_run(0, k, r, L, nconn, 20000, batch, 2000, 2, 0.0, REG | PER_CONN, warm)
    res = {"tag": args.tag}
    for leg, ragged, recover in (("ragged_generate", 1, 0), ("ragged_recover", 1, 1), ("equal_generate", 0, 0),
                                 ("equal_recover", 0, 1)):
        lib.bl_set_ragged(1500 if ragged else 0, 20261019)
        out, rows, ph, q = (C.c_double * 8)(), (C.c_double * 2)(), (C.c_double * 6)(), (C.c_double * 8)()
        if recover:
            rc = lib.bl_run_recover(0, k, r, L, e, nconn, args.blocks, batch, 2000, 2, REG | PER_CONN, out)
        else:
            rc = lib.bl_run(0, k, r, L, nconn, args.blocks, batch, 2000, 2, 0.0, REG | PER_CONN, out)
        lib.bl_last_rows(rows)
        lib.bl_last_phases(ph)
        lib.bl_last_latency(q)
        res[leg] = {"rc": rc, "payload_GiB_s": round(out[0], 2), "p50_us": out[1], "p99_us": out[2],
                    "rows_in_place": int(rows[0]), "rows_staged": int(rows[1]), "stage_us": int(ph[1]),
                    "engine_us": int(ph[0])}
    lib.bl_set_ragged(0, 0)
    print(json.dumps(res), flush=True)


def quartiles(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4, method="inclusive")
    return q[0], statistics.median(xs), q[2]


def mode_summary():
    runs = {}
    for path in (args.a, args.b):
        for line in open(path):
            line = line.strip()
            if line.startswith("{"):
                j = json.loads(line)
                runs.setdefault(j["tag"], []).append(j)
    tags = list(runs)
    assert len(tags) == 2, tags
    base, head = tags
    legs = [x for x in runs[base][0] if x != "tag"]
    for leg in legs:
        print(leg)
        med = {}
        for t in tags:
            rs = [x[leg] for x in runs[t] if x[leg]["rc"] == 0]
            g = [x["payload_GiB_s"] for x in rs]
            q1, m, q3 = quartiles(g)
            med[t] = (m, q3 - q1)
            p99 = statistics.median(x["p99_us"] for x in rs)
            print(f"  {t:7s} {len(rs):2d} runs  payload GiB/s median {m:6.2f}  quartiles {q1:6.2f} - {q3:6.2f}  "
                  f"(min {min(g):.2f}, max {max(g):.2f})  p99 median {p99:7.0f} us  "
                  f"rows in place / staged {rs[0]['rows_in_place']} / {rs[0]['rows_staged']}  "
                  f"stage_us median {statistics.median(x['stage_us'] for x in rs):.0f}")
        (mb, iqr), (mh, _) = med[base], med[head]
        ok = mh >= mb - iqr
        print(f"  {head} - {base} median {mh - mb:+.2f} GiB/s; bar: not below {base}'s median by more than its "
              f"inter-quartile spread {iqr:.2f}: {'within' if ok else 'BELOW'} the bar")


{"device": mode_device, "copies": mode_copies, "load": mode_load, "summary": mode_summary}[args.mode]()
