"""What full-rank recovery costs in the layers above the packed decode, both modes interleaved in one
process on the same buffers; medians with min-max.

 1. one block through the resident block service, reference request against full-rank request, and
    fecgpu_rlc_decode_host_full on one block beside them, as it routes the block and with knob plan 1
    (plan + fix-up + apply, three launches): a block reference mode recovers, one it gives up on, a
    singular one; k16 r6 and k32 r8, L 1200
 2. small batches (1, 8, 64 blocks) of fecgpu_rlc_decode_full: the one-launch path against plan + fix-up +
    apply (knob plan 1)
 3. fecgpu_rlc_decode_rows_fused_full against fecgpu_rlc_decode_rows_fused, k16 r4 e4 L1200, 2^16 blocks,
    the bench's erasure generator; bar: reference median x (1 + share of extra blocks) + reference spread
With PQUIC_AMD_LIB set to an older build of the library (A/B baselines) the parts it lacks are left out:
what remains is that build's three-launch full path.
usage: python tools/full_rank_layers.py [--repeats N]   (writes nothing: redirect into profiles/)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pquic_amd import BLOCK_RECOVERED, BLOCK_REF_UB, BLOCK_SINGULAR, Engine, HostPath, load_library  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=200)
args = ap.parse_args()

eng = Engine(0)
lib = load_library()
dev = torch.device("cuda:0")
HAS_LAYERS = hasattr(lib, "fecgpu_block_svc_rlc_decode_full")
print("library:", os.environ.get("PQUIC_AMD_LIB") or "this tree's", "" if HAS_LAYERS else "(no full-rank layers)")


def med_range(xs):
    return f"{statistics.median(xs):9.1f} us  ({min(xs):.1f} - {max(xs):.1f})"


def batch(k, r, e, L, nb, seed):
    """nb blocks with e random erasures each and every repair received; statuses of both modes."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    miss = torch.rand((nb, k), generator=g).argsort(dim=1)[:, :e]
    pres = torch.ones((nb, k), dtype=torch.bool)
    pres.scatter_(1, miss, False)
    sp = torch.zeros((nb, 2), dtype=torch.int64)
    for j in range(k):
        sp[:, j >> 6] |= pres[:, j].to(torch.int64) << (j & 63)
    rp = torch.zeros((nb, 2), dtype=torch.int64)
    rp[:, 0] = (1 << r) - 1
    src = torch.empty((nb, k, L), dtype=torch.uint8, device=dev)
    eng.synth_fill(src, src.numel(), 0x5EEDF3C0 + seed, 0)
    rep = torch.empty((nb, r, L), dtype=torch.uint8, device=dev)
    eng.rlc_encode(src, rep, k, r, L, nblocks=nb)
    work = src.clone()
    work.view(nb * k, L)[(torch.arange(nb).unsqueeze(1) * k + miss).reshape(-1).to(dev)] = 0xA5
    sp, rp = sp.to(dev), rp.to(dev)
    st = {m: torch.empty(nb, dtype=torch.uint8, device=dev) for m in ("ref", "full")}
    rec = torch.empty((nb, 2), dtype=torch.int64, device=dev)
    eng.rlc_decode(work.clone(), rep, sp, rp, st["ref"], rec, k, r, L, nblocks=nb)
    eng.rlc_decode_full(work.clone(), rep, sp, rp, st["full"], rec, k, r, L, nblocks=nb)
    torch.cuda.synchronize()
    return dict(k=k, r=r, e=e, L=L, nb=nb, src=src, rep=rep, work=work, sp=sp, rp=rp, st_ref=st["ref"].cpu().numpy(),
                st_full=st["full"].cpu().numpy())


def pin(t):
    return t.cpu().contiguous().pin_memory()


# ---------------------------------------------------------------------------------------- 1. block service
def service(k, r, L):
    B = batch(k, r, r, L, 8192, 31)
    kinds = {"reference recovers": np.nonzero(B["st_ref"] == BLOCK_RECOVERED)[0],
             "reference gives up": np.nonzero((B["st_ref"] == BLOCK_REF_UB) & (B["st_full"] == BLOCK_RECOVERED))[0],
             "singular": np.nonzero(B["st_full"] == BLOCK_SINGULAR)[0]}
    svc = lib.fecgpu_block_svc_create(0)
    lib.fecgpu_block_svc_set_deadline(svc, 1_000_000)
    hp = HostPath(0, 1, 1 << 20)
    print(f"block service, one block per call, k{k} r{r} e{r} L{L}, {args.repeats} interleaved repeats")
    for kind, idx in kinds.items():
        if idx.size == 0:
            print(f"  {kind}: no such block among {B['nb']}")
            continue
        b = int(idx[0])
        work0, rep = pin(B["work"][b:b + 1]), pin(B["rep"][b:b + 1])
        work = work0.clone().pin_memory()
        seeds = pin(torch.tensor([(b << 8) | i for i in range(r)], dtype=torch.int32))
        sp, rpm = pin(B["sp"][b:b + 1]), pin(B["rp"][b:b + 1])
        st = torch.zeros(16, dtype=torch.uint8).pin_memory()
        rec = torch.zeros((1, 2), dtype=torch.int64).pin_memory()
        a = (work.data_ptr(), rep.data_ptr(), work.data_ptr(), k, r, L, seeds.data_ptr(), sp.data_ptr(),
             rpm.data_ptr(), st.data_ptr(), rec.data_ptr())
        def host_full(plan):
            with eng.knob("plan", plan):
                hp.rlc_decode_full(work, rep, sp, rpm, st, rec, 1, k, r, L, seeds=seeds)

        calls = {"service, reference": lambda: lib.fecgpu_block_svc_rlc_decode_seeded(svc, *a)}
        if HAS_LAYERS:
            calls["service, full rank"] = lambda: lib.fecgpu_block_svc_rlc_decode_full(svc, *a)
        calls["host path, full"] = lambda: host_full(0)
        calls["host path, full, plan 1"] = lambda: host_full(1)
        t = {n: [] for n in calls}
        status = {}
        for it in range(args.repeats + 20):
            for n, f in calls.items():
                work.copy_(work0)
                t0 = time.perf_counter()
                rc = f()
                dt = (time.perf_counter() - t0) * 1e6
                assert not rc, (n, rc)
                status[n] = int(st[0])
                if it >= 20:
                    t[n].append(dt)
        print(f"  {kind} (block {b}):")
        for n in calls:
            print(f"    {n:24s} status {status[n]}  {med_range(t[n])}")
    lib.fecgpu_block_svc_destroy(svc)
    hp.close()


# ---------------------------------------------------------------------------------------- 2. small batches
def small_batches(k, r, L):
    B = batch(k, r, r, L, 8192, 32)
    pick = np.nonzero((B["st_ref"] == BLOCK_REF_UB) & (B["st_full"] == BLOCK_RECOVERED))[0]
    ok = np.nonzero(B["st_ref"] == BLOCK_RECOVERED)[0]
    print(f"small batches of fecgpu_rlc_decode_full, k{k} r{r} e{r} L{L}: one launch against plan + fix-up + apply")
    for nb in (1, 8, 64):
        # one block in eight is one reference mode gives up on (far above the natural share), the rest it recovers
        idx = np.array([pick[x % pick.size] if x % 8 == 0 else ok[x] for x in range(nb)])
        ti = torch.from_numpy(idx).to(dev)
        work0, rep = B["work"][ti].contiguous(), B["rep"][ti].contiguous()
        sp, rp = B["sp"][ti].contiguous(), B["rp"][ti].contiguous()
        fbn = ti.to(torch.int32)
        work = work0.clone()
        st = torch.empty(nb, dtype=torch.uint8, device=dev)
        rec = torch.empty((nb, 2), dtype=torch.int64, device=dev)
        ws = eng.alloc_workspace(nb, k, r)
        t = {"one launch": [], "three launches": []}
        for it in range(args.repeats + 20):
            for n in t:
                work.copy_(work0)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                with eng.knob("plan", 0 if n == "one launch" else 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ev[0].record()
                    eng.lib.fecgpu_rlc_decode_full(work.data_ptr(), rep.data_ptr(), nb, k, r, L, 0, fbn.data_ptr(), None,
                                                   sp.data_ptr(), rp.data_ptr(), st.data_ptr(), rec.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), None)
                    ev[1].record()
                    ev[1].synchronize()
                    wall = (time.perf_counter() - t0) * 1e6
                if it >= 20:
                    t[n].append((ev[0].elapsed_time(ev[1]) * 1e3, wall))
            assert bool((st == BLOCK_RECOVERED).all())
        for n, v in t.items():
            print(f"  {nb:3d} blocks  {n:15s} device {med_range([x[0] for x in v])}   call to completion "
                  f"{med_range([x[1] for x in v])}")


# ---------------------------------------------------------------------------------------- 3. rows
def rows(k, r, e, L, nb, repeats):
    B = batch(k, r, e, L, nb, 11)
    base_s, base_r, base_w = B["src"].data_ptr(), B["rep"].data_ptr(), B["work"].data_ptr()
    srow = (base_w + torch.arange(nb * k, dtype=torch.int64) * L).to(dev)
    rrow = (base_r + torch.arange(nb * r, dtype=torch.int64) * L).to(dev)
    slen = torch.full((nb * k,), L, dtype=torch.int32, device=dev)
    rlen = torch.full((nb * r,), L, dtype=torch.int32, device=dev)
    blen = torch.full((nb,), L, dtype=torch.int32, device=dev)
    seeds = ((torch.arange(nb, dtype=torch.int64).unsqueeze(1) << 8) | torch.arange(r)).to(torch.int32).to(dev)
    ws = eng.alloc_workspace(nb, k, r)
    out = {m: (torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty((nb, 2), dtype=torch.int64, device=dev))
           for m in ("ref", "full")}
    f = {"ref": eng.rlc_decode_rows_fused, "full": eng.rlc_decode_rows_fused_full}
    t = {"ref": [], "full": []}
    for it in range(repeats + 3):
        for m in t:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            f[m](srow, slen, rrow, rlen, blen, seeds, B["sp"], B["rp"], *out[m], nb, k, r, L, workspace=ws)
            ev[1].record()
            ev[1].synchronize()
            if it >= 3:
                t[m].append(ev[0].elapsed_time(ev[1]) * 1e3)
    n_ref = int((out["ref"][0] == BLOCK_RECOVERED).sum())
    n_full = int((out["full"][0] == BLOCK_RECOVERED).sum())
    okb = (out["full"][0] == BLOCK_RECOVERED)
    assert bool((B["work"][okb] == B["src"][okb]).all()), "recovered rows differ"
    extra = (n_full - n_ref) / n_ref
    ref_med, full_med = statistics.median(t["ref"]), statistics.median(t["full"])
    spread = max(t["ref"]) - min(t["ref"])
    bar = ref_med * (1 + extra) + spread
    print(f"rows_fused against rows_fused_full, k{k} r{r} e{e} L{L}, {nb} blocks, {repeats} interleaved repeats")
    print(f"  recovered: reference {n_ref}, full {n_full} (+{n_full - n_ref} blocks, +{100 * extra:.2f} %), singular "
          f"{int((out['full'][0] == BLOCK_SINGULAR).sum())}; full-mode rows equal the sources")
    for m in t:
        print(f"  {m:4s} {med_range(t[m])}")
    verdict = "within the bar" if full_med <= bar else f"OVER the bar by {full_med - bar:.1f} us"
    print(f"  full - ref {full_med - ref_med:+.1f} us ({100 * (full_med / ref_med - 1):+.2f} %); bar {bar:.1f} us = "
          f"ref {ref_med:.1f} x (1 + {extra:.4f}) + ref spread {spread:.1f}: {verdict}", flush=True)
    del base_s


service(16, 6, 1200)
service(32, 8, 1200)
if HAS_LAYERS:
    small_batches(16, 6, 1200)
    small_batches(32, 8, 1200)
    rows(16, 4, 4, 1200, 1 << 16, 30)
