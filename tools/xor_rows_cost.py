"""What XOR on rows costs and saves: the figures of profiles/xor_rows.log.

  device   k4 and k16, L1200, 2^16 blocks on device-resident rows, interleaved in one process on the same
           buffers, timed with events: (a) fecgpu_xor_encode / fecgpu_xor_decode_to on the packed rows,
           (b) fecgpu_xor_encode_rows / fecgpu_xor_decode_rows on the same rows with every length equal,
           (c) the three-pass composition: fecgpu_rows_gather + (a) + fecgpu_rows_scatter; then (b) and (c)
           again on ragged lengths.  Hard condition: (b)'s median below (c)'s minimum, both directions,
           both length cases (exit status 1 otherwise).  (b) / (a) is reported with the min-max of both.
  lanes    the row forms alone on device rows and on page-locked host rows, equal and ragged lengths: the
           A/B behind the kept geometry, one line set per library build (PQUIC_AMD_LIB selects a build
           with another -DFEC_XOR_ROWS_LPB, or -DFEC_XOR_ROWS_KC=0: no compile-time-k variants).
  load     ONE run of each batcher leg through tools/libbatchload.so (or --loadlib: the same generator
           linked against another tree's engine): XOR generate and recover, k4 r1, 64 connections with
           registered arenas, equal lengths (L1200, max_symbol 1200) and ragged (max_symbol 1500,
           1200-byte blocks of ragged packets), and the RLC equal-length generate and recover legs of
           bench.py's batch_saturated.  Prints one JSON line; run it alternately per tree.
  summary  medians and quartiles of the JSON lines of two trees (files given as --a / --b), and the bars:
           head's median payload rate not below the parent's median minus its inter-quartile range, head's
           p99 not above the parent's plus its inter-quartile range.
usage: python tools/xor_rows_cost.py device|lanes|load|summary [options]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["device", "lanes", "load", "summary"])
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--loadlib", default=os.path.join(ROOT, "tools", "libbatchload.so"))
ap.add_argument("--tag", default="head")
ap.add_argument("--blocks", type=int, default=200000)
ap.add_argument("--a")
ap.add_argument("--b")
args = ap.parse_args()

L, NB = 1200, 1 << 16


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


def ragged_lengths(torch, nb, k, dev):
    """One source of every block full, the others uniform in [40, L] (seeded)."""
    n = torch.randint(40, L + 1, (nb, k), generator=torch.Generator().manual_seed(7)).to(torch.int32)
    n[torch.arange(nb), torch.arange(nb) % k] = L
    return n.reshape(-1).to(dev)


class Rows:
    """k source rows and one repair row per block in `base` memory (a device tensor's or a page-locked
    buffer's device address), with their tables, and the masks of a batch that lost source b % k."""

    def __init__(self, torch, dev, k, nb, src_base, rep_base):
        self.k, self.nb = k, nb
        self.srow = src_base + torch.arange(nb * k, dtype=torch.int64, device=dev) * L
        self.rrow = rep_base + torch.arange(nb, dtype=torch.int64, device=dev) * L
        self.miss = torch.arange(nb, device=dev) % k
        self.mrow = self.srow.reshape(nb, k)[torch.arange(nb, device=dev), self.miss].contiguous()
        self.sp = torch.zeros((nb, 2), dtype=torch.int64, device=dev)
        self.sp[:, 0] = ((1 << k) - 1) & ~(1 << self.miss)
        self.rp = torch.zeros((nb, 2), dtype=torch.int64, device=dev)
        self.rp[:, 0] = 1
        self.st = torch.empty(nb, dtype=torch.uint8, device=dev)
        self.rec = torch.empty((nb, 2), dtype=torch.int64, device=dev)
        self.blen = torch.full((nb,), L, dtype=torch.int32, device=dev)
        self.lens = {"equal": torch.full((nb * k,), L, dtype=torch.int32, device=dev),
                     "ragged": ragged_lengths(torch, nb, k, dev)}


def mode_device():
    import torch
    from pquic_amd import Engine
    eng = Engine(0)
    dev = torch.device("cuda:0")
    failed = False
    for k in (4, 16):
        nb = NB
        src = torch.empty((nb, k, L), dtype=torch.uint8, device=dev)
        eng.synth_fill(src, src.numel(), 0x5EEDF3C0, 0)
        rep = torch.empty((nb, 1, L), dtype=torch.uint8, device=dev)
        R = Rows(torch, dev, k, nb, src.data_ptr(), rep.data_ptr())
        psrc, prep, pdst = torch.empty_like(src), torch.empty_like(rep), torch.empty_like(rep)
        rep_c = torch.empty_like(rep)  # (c)'s repairs, beside (b)'s
        rrow_c = rep_c.data_ptr() + torch.arange(nb, dtype=torch.int64, device=dev) * L

        def a_enc():
            eng.xor_encode(src, rep, k, L)

        def a_dec():
            eng.xor_decode_to(src, rep, pdst, R.sp, R.rp, R.st, R.rec, k, L)

        def b_enc(slen, rrow=None):
            eng.xor_encode_rows(R.srow, slen, R.rrow if rrow is None else rrow, R.blen, nb, k, L)

        def b_dec(slen):
            eng.xor_decode_rows(R.srow, slen, R.rrow, R.blen, R.sp, R.rp, R.st, R.rec, nb, k, L)

        def c_enc(slen, rrow=None):
            eng.rows_gather(R.srow, slen, nb * k, L, psrc)
            eng.xor_encode(psrc, prep, k, L)
            eng.rows_scatter(prep, R.rrow if rrow is None else rrow, R.blen, nb, L)

        def c_dec(slen):
            eng.rows_gather(R.srow, slen, nb * k, L, psrc)
            eng.rows_gather(R.rrow, R.blen, nb, L, prep)
            eng.xor_decode_to(psrc, prep, pdst, R.sp, R.rp, R.st, R.rec, k, L)
            eng.rows_scatter(pdst, R.mrow, R.blen, nb, L)

        # the three agree before anything is timed: equal lengths against the packed kernel, ragged (b) against (c)
        a_enc()
        keep = rep.clone()
        rep.zero_()
        b_enc(R.lens["equal"])
        torch.cuda.synchronize()
        assert torch.equal(rep, keep), "xor_encode_rows differs from xor_encode"
        orig = src.clone()
        b_dec(R.lens["equal"])
        torch.cuda.synchronize()
        assert torch.equal(src, orig) and int(R.st.max()) == 0, "xor_decode_rows does not give the source back"
        b_enc(R.lens["ragged"])
        c_enc(R.lens["ragged"], rrow_c)
        torch.cuda.synchronize()
        assert torch.equal(rep, rep_c), "ragged: xor_encode_rows differs from gather + xor_encode + scatter"
        a_enc()

        print(f"k{k} L{L}, {nb} blocks, device-resident rows, {args.repeats} interleaved repeats")
        for lname in ("equal", "ragged"):
            sl = R.lens[lname]
            fns = {"b_encode_rows": lambda: b_enc(sl), "c_gather_encode_scatter": lambda: c_enc(sl),
                   "b_decode_rows": lambda: b_dec(sl), "c_gather_decode_scatter": lambda: c_dec(sl)}
            if lname == "equal":
                fns = {"a_encode_packed": a_enc, "a_decode_to_packed": a_dec, **fns}
            t = timed(fns, args.repeats)
            payload = int(sl.sum())
            print(f" {lname} lengths ({payload / (nb * k):.0f} B per source on average)")
            for n, xs in t.items():
                print(f"  {n:24s} {med_range(xs)}  {payload / statistics.median(xs) / 1073.741824:8.1f} GiB/s payload")
            for bname, cname in (("b_encode_rows", "c_gather_encode_scatter"),
                                 ("b_decode_rows", "c_gather_decode_scatter")):
                ok = statistics.median(t[bname]) < min(t[cname])
                failed |= not ok
                print(f"  {bname} median {statistics.median(t[bname]):.1f} us against {cname} minimum "
                      f"{min(t[cname]):.1f} us: {'below, as required' if ok else 'NOT BELOW'}")
            if lname == "equal":
                for bname, aname in (("b_encode_rows", "a_encode_packed"), ("b_decode_rows", "a_decode_to_packed")):
                    ma, mb = statistics.median(t[aname]), statistics.median(t[bname])
                    print(f"  {bname} / {aname}: x{mb / ma:.3f}  (a spread {(max(t[aname]) - min(t[aname])) / ma:.1%}, "
                          f"tables {(12 * k + 16) / ((k + 1) * L):.1%} of the bytes)", flush=True)
        del src, rep, psrc, prep, pdst, rep_c, keep, orig, R
        torch.cuda.empty_cache()
    sys.exit(1 if failed else 0)


def mode_lanes():
    import torch
    from pquic_amd import Engine
    from pquic_amd.engine import LIB_PATH
    eng = Engine(0)
    dev = torch.device("cuda:0")
    eng.lib.fecgpu_host_alloc.restype = C.c_void_p
    eng.lib.fecgpu_host_alloc.argtypes = [C.c_size_t]
    eng.lib.fecgpu_host_free.argtypes = [C.c_void_p]
    print(f"library {os.path.relpath(LIB_PATH, ROOT)}: XOR row forms, {NB} blocks of L{L}")
    for k in (4, 16):
        nb = NB
        src = torch.empty((nb, k, L), dtype=torch.uint8, device=dev)
        eng.synth_fill(src, src.numel(), 0x5EEDF3C0, 0)
        rep = torch.empty((nb, 1, L), dtype=torch.uint8, device=dev)
        nbytes = nb * (k + 1) * L
        host = eng.lib.fecgpu_host_alloc(nbytes)
        assert host
        C.memset(host, 0x5A, nbytes)
        d = C.c_uint64(0)
        assert eng.lib.fecgpu_host_device_address(host, nbytes, C.byref(d)) == 0
        for where, sb, rb in (("device rows", src.data_ptr(), rep.data_ptr()),
                              ("page-locked host rows", d.value, d.value + nb * k * L)):
            R = Rows(torch, dev, k, nb, sb, rb)
            for lname, sl in R.lens.items():
                enc = lambda: eng.xor_encode_rows(R.srow, sl, R.rrow, R.blen, nb, k, L)  # noqa: E731
                dec = lambda: eng.xor_decode_rows(R.srow, sl, R.rrow, R.blen, R.sp, R.rp, R.st, R.rec, nb, k, L)  # noqa: E731
                t = timed({"encode": enc, "decode": dec}, args.repeats)
                moved = {"encode": int(sl.sum()) + nb * L, "decode": int(sl.sum()) + nb * L}
                for name, xs in t.items():
                    print(f"  k{k:<2d} {where:22s} {lname:6s} {name:6s} {med_range(xs)}  "
                          f"{moved[name] / statistics.median(xs) / 1073.741824:7.1f} GiB/s moved", flush=True)
        eng.lib.fecgpu_host_free(host)
        del src, rep
        torch.cuda.empty_cache()


def mode_load():
    lib = C.CDLL(args.loadlib)
    D = C.POINTER(C.c_double)
    lib.bl_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_uint, C.c_uint, C.c_int,
                           C.c_double, C.c_int, D]
    lib.bl_run_recover.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_uint,
                                   C.c_uint, C.c_int, C.c_int, D]
    lib.bl_set_inflight.argtypes = [C.c_int]
    lib.bl_set_ragged.argtypes = [C.c_int, C.c_uint]
    lib.bl_set_xor.argtypes = [C.c_int]
    for f in ("bl_last_rows", "bl_last_phases", "bl_last_latency"):
        getattr(lib, f).argtypes = [D]
    REG, PER_CONN = 1, 2
    nconn, batch = 64, 2048  # bench.py's batch_saturated legs
    lib.bl_set_inflight(3)
    warm = (C.c_double * 8)()
    lib.bl_run(0, 16, 4, L, nconn, 20000, batch, 2000, 2, 0.0, REG | PER_CONN, warm)
    res = {"tag": args.tag}
    legs = (("xor_equal_generate", 1, 0, 0), ("xor_equal_recover", 1, 0, 1), ("xor_ragged_generate", 1, 1, 0),
            ("xor_ragged_recover", 1, 1, 1), ("rlc_equal_generate", 0, 0, 0), ("rlc_equal_recover", 0, 0, 1))
    for leg, xor, ragged, recover in legs:
        k, r, e = (4, 1, 1) if xor else (16, 4, 4)
        lib.bl_set_xor(xor)
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
    lib.bl_set_xor(0)
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
    bad = False
    for leg in legs:
        print(leg)
        rate, p99 = {}, {}
        for t in tags:
            rs = [x[leg] for x in runs[t] if x[leg]["rc"] == 0]
            q1, m, q3 = quartiles([x["payload_GiB_s"] for x in rs])
            l1, lm, l3 = quartiles([x["p99_us"] for x in rs])
            rate[t], p99[t] = (m, q3 - q1), (lm, l3 - l1)
            g = [x["payload_GiB_s"] for x in rs]
            print(f"  {t:7s} {len(rs):2d} runs  payload GiB/s median {m:6.2f}  quartiles {q1:6.2f} - {q3:6.2f}  "
                  f"(min {min(g):.2f}, max {max(g):.2f})  p99 median {lm:7.0f} us  quartiles {l1:.0f} - {l3:.0f}  "
                  f"rows in place / staged {rs[0]['rows_in_place']} / {rs[0]['rows_staged']}  "
                  f"stage_us median {statistics.median(x['stage_us'] for x in rs):.0f}")
        ok_r = rate[head][0] >= rate[base][0] - rate[base][1]
        ok_l = p99[head][0] <= p99[base][0] + p99[base][1]
        bad |= not (ok_r and ok_l)
        print(f"  {head} - {base}: payload median {rate[head][0] - rate[base][0]:+.2f} GiB/s "
              f"(x{rate[head][0] / rate[base][0]:.2f}; bar: not below {base}'s median minus its inter-quartile range "
              f"{rate[base][1]:.2f}: {'within' if ok_r else 'BELOW'}); p99 median {p99[head][0] - p99[base][0]:+.0f} us "
              f"(bar: not above {base}'s plus its inter-quartile range {p99[base][1]:.0f}: "
              f"{'within' if ok_l else 'ABOVE'})")
    sys.exit(1 if bad else 0)


{"device": mode_device, "lanes": mode_lanes, "load": mode_load, "summary": mode_summary}[args.mode]()
