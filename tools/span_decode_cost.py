"""What the span decode costs next to decoding the same received symbols window by window: both variants in
one process on the same device buffers, interleaved, timed with events.

Workloads: the window shapes bench.py uses (k30 r1 step 5, k30 r5 step 25, k32 r8 step 8), 2^16 spans of as
many whole windows as 128 columns and 128 repair slots hold, L 1200, independent loss of sources and repairs.
  span     fecgpu_rlc_span_decode_plan + fecgpu_rlc_decode_apply_packed, one record per span
  windows  full-rank mode per window, one block per (span, window) with its own repairs only.  The windows
           overlap in the stream, so they are decoded where they lie, through the row form of the same mode
           (fecgpu_rlc_decode_rows_full, in the parent commit): no symbol is copied into per-window blocks,
           which favours this variant.  Its input masks are those of the received symbols (no window sees
           what another recovered).
  rows     fecgpu_rlc_span_decode_rows_fused on the same buffers, every row by address with its length (the
           form the batching adapter's span jobs use)
The span and rows variants run with knob span_compact at 0 and at 1 (the compacted data pass), all in the same
interleaved loop.  The packed variant's 16-unknown tiles take the LDS-ring kernel, which the knob does not
reach; the row form never takes the ring.
Per shape and loss: the span plan kernel alone, every variant's total (median, min-max over the repeats),
symbols recovered, microseconds per recovered symbol, and the share of rows the compacted data pass lists
(from the plan records: per tile of 16 unknowns, the input slots with a non-zero coefficient, over K).
usage: python tools/span_decode_cost.py [--repeats N] [--loss P ...] [--small]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pquic_amd import BLOCK_RECOVERED, Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--loss", type=float, nargs="+", default=[0.01, 0.03])
ap.add_argument("--small", action="store_true", help="1/16 of the spans (a quick look, not the committed figures)")
args = ap.parse_args()

eng = Engine(0)
dev = torch.device("cuda:0")


def masks(present):
    """(n, width <= 128) bool on the device -> (n, 2) int64 presence masks"""
    n, w = present.shape
    p = torch.zeros((n, 128), dtype=torch.bool, device=dev)
    p[:, :w] = present
    out = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    for x in range(2):
        b = p[:, 64 * x: 64 * x + 64].to(torch.int64)
        out[:, x] = (b[:, :63] << torch.arange(63, dtype=torch.int64, device=dev)).sum(1) | (b[:, 63] << 63)
    return out


def bits(m, n):
    j = torch.arange(n, device=dev)
    return ((m[:, j >> 6] >> (j & 63)) & 1).bool()


def med_range(xs):
    return f"{statistics.median(xs):10.1f} us  ({min(xs):.1f} - {max(xs):.1f})"


def pad16(x):
    return (x + 15) & ~15


def rows_listed(ws, nb, K, R, tile=16):
    """Share of the K input slots the compacted setup lists, over every tile of `tile` unknowns of the plan
    records in ws (the workspace layout of fec_engine.hip: header, unknowns, selection, slots, flags, D)."""
    em = min(K, R)
    off_d = 16 + 3 * pad16(em) + pad16(K)
    stride = off_d + pad16(em * K) + pad16(em * em)
    rec = ws[:nb * stride].view(nb, stride)
    ok = rec[:, 0] == BLOCK_RECOVERED
    e = torch.where(ok, rec[:, 1], torch.zeros_like(rec[:, 1])).to(torch.int64)
    listed = tiles = 0
    for r0 in range(0, em, tile):
        n = min(tile, em - r0)
        d = rec[:, off_d + r0 * K: off_d + (r0 + n) * K].view(nb, n, K) != 0
        live = (torch.arange(r0, r0 + n, device=dev).unsqueeze(0) < e.unsqueeze(1)).unsqueeze(2)
        listed += int((d & live).any(1).sum())
        tiles += int((e > r0).sum())
    return listed / max(tiles * K, 1), tiles


def workload(k, r, step, L, nb, loss):
    W = min((128 - k) // step + 1, 128 // r)
    K, R = k + (W - 1) * step, W * r
    src = torch.empty((nb, K, L), dtype=torch.uint8, device=dev)
    eng.synth_fill(src, src.numel(), 0x5EED5BA9, 0)
    rep = torch.empty((nb, R, L), dtype=torch.uint8, device=dev)
    stream = src.view(nb * K, L)
    tmp = torch.empty((nb, r, L), dtype=torch.uint8, device=dev)
    for w in range(W):  # window w of every span: the spans' columns are one stream, K symbols apart
        eng.rlc_window_encode(stream[w * step:], tmp, nb, K, k, r, L)
        rep[:, w * r:(w + 1) * r] = tmp
    del tmp
    g = torch.Generator(device="cpu").manual_seed(17)
    present = (torch.rand((nb, K), generator=g) >= loss).to(dev)
    rpresent = (torch.rand((nb, R), generator=g) >= loss).to(dev)
    sp, rp = masks(present), masks(rpresent)
    seed = torch.arange(r, dtype=torch.int32, device=dev).repeat(W).repeat(nb, 1).contiguous()
    off = (torch.arange(W, device=dev) * step).repeat_interleave(r).to(torch.uint8).repeat(nb, 1).contiguous()
    nss = torch.full((nb, R), k, dtype=torch.uint8, device=dev)
    work = torch.where(present.unsqueeze(2), src, torch.tensor(0xA5, dtype=torch.uint8, device=dev))
    lost = int((~present).sum())
    # span variant
    em = min(K, R)
    ws = eng.alloc_workspace(nb, K, R)
    dst = torch.empty((nb, em, L), dtype=torch.uint8, device=dev)
    st = torch.empty(nb, dtype=torch.uint8, device=dev)
    rec = torch.empty((nb, 2), dtype=torch.int64, device=dev)
    # window variant: block (span b, window w) = rows b*K + w*step .. + k of the span buffer, repairs w*r .. + r
    nw = nb * W
    base = (torch.arange(nb, device=dev).unsqueeze(1) * K + torch.arange(W, device=dev).unsqueeze(0) * step).reshape(-1)
    wwork = work.clone()
    srow = (wwork.data_ptr() + (base.unsqueeze(1) + torch.arange(k, device=dev).unsqueeze(0)) * L).contiguous()
    rrow = (rep.data_ptr() + torch.arange(nb * R, device=dev) * L).contiguous()  # slot order is window order
    cols = (torch.arange(W, device=dev) * step).unsqueeze(1) + torch.arange(k, device=dev).unsqueeze(0)  # (W, k)
    wsp = masks(present[:, cols].reshape(nw, k))
    wrp = masks(rpresent.reshape(nw, r))
    wseed = torch.arange(r, dtype=torch.int32, device=dev).repeat(nw, 1).contiguous()
    wws = eng.alloc_workspace(nw, k, r)
    wst = torch.empty(nw, dtype=torch.uint8, device=dev)
    wrec = torch.empty((nw, 2), dtype=torch.int64, device=dev)

    # row form: the span buffers' rows by address, every length L; its own copy of the received rows, since
    # it decodes in place
    rwork = work.clone()
    f_srow = (rwork.data_ptr() + torch.arange(nb * K, device=dev) * L).contiguous()
    f_len = torch.full((nb * K,), L, dtype=torch.int32, device=dev)
    f_rlen = torch.full((nb * R,), L, dtype=torch.int32, device=dev)
    f_blen = torch.full((nb,), L, dtype=torch.int32, device=dev)
    fws = eng.alloc_workspace(nb, K, R)
    fst = torch.empty(nb, dtype=torch.uint8, device=dev)
    frec = torch.empty((nb, 2), dtype=torch.int64, device=dev)

    def rows(compact, ev=None):
        eng.set_knob("span_compact", compact)
        if ev:
            ev[0].record()
        eng.rlc_span_decode_rows_fused(f_srow, f_len, rrow, f_rlen, f_blen, seed, off, nss, sp, rp, fst, frec, nb, K, R,
                                       L, workspace=fws)
        if ev:
            ev[2].record()

    def span(compact=1, ev=None):
        eng.set_knob("span_compact", compact)
        if ev:
            ev[0].record()
        eng.rlc_span_decode_plan(seed, off, nss, sp, rp, K, R, nb, ws)
        if ev:
            ev[1].record()
        eng.rlc_decode_apply_packed(work, rep, dst, st, rec, K, R, L, nb, ws)
        if ev:
            ev[2].record()

    def windows(ev=None):
        if ev:
            ev[0].record()
        eng.rlc_decode_rows_full(srow, rrow, wseed, wsp, wrp, wst, wrec, nw, k, r, L, workspace=wws)
        if ev:
            ev[2].record()

    for _ in range(2):
        for c in (0, 1):
            span(c)
            rows(c)
            rwork.copy_(work)
        windows()
        wwork.copy_(work)
    torch.cuda.synchronize()
    t = {"plan": [], "span0": [], "span": [], "rows0": [], "rows1": [], "windows": []}
    for _ in range(args.repeats):  # interleaved: drift hits every variant alike
        for c in (0, 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            span(c, ev)
            ev[2].synchronize()
            if c:
                t["plan"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            t["span" if c else "span0"].append(ev[0].elapsed_time(ev[2]) * 1e3)
            rwork.copy_(work)  # the row form decodes in place: every repeat starts from the received rows
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            rows(c, ev)
            ev[2].synchronize()
            t[f"rows{c}"].append(ev[0].elapsed_time(ev[2]) * 1e3)
        wwork.copy_(work)  # the window variant decodes in place: every repeat starts from the received rows
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        windows(ev)
        ev[2].synchronize()
        t["windows"].append(ev[0].elapsed_time(ev[2]) * 1e3)
    # what each variant recovered; the span variant's rows against the sources
    det = bits(rec, K) & ~present
    n_span = int(det.sum())
    share, tiles = rows_listed(ws, nb, K, R)
    assert bool((fst == st).all()) and bool((frec == rec).all()), "row form: status / recovered differ"
    for c0 in range(0, nb, 2048):
        same = (rwork[c0:c0 + 2048] == src[c0:c0 + 2048]).all(2)
        assert bool((same == (present[c0:c0 + 2048] | det[c0:c0 + 2048])).all()), "row form rows differ"
    eng.rlc_span_decode(work, rep, seed, off, nss, sp, rp, st, rec, K, R, L, nspans=nb, workspace=ws)
    torch.cuda.synchronize()
    for c0 in range(0, nb, 2048):
        same = (work[c0:c0 + 2048] == src[c0:c0 + 2048]).all(2)
        assert bool((same == (present[c0:c0 + 2048] | det[c0:c0 + 2048])).all()), "span decode rows differ"
    wdet = torch.zeros((nb, K), dtype=torch.bool, device=dev)
    got = bits(wrec, k).reshape(nb, W, k)
    for w in range(W):
        wdet[:, w * step:w * step + k] |= got[:, w]
    wdet &= ~present
    n_win = int(wdet.sum())
    assert bool((wdet & ~det).sum() == 0), "a window recovered what the span decode did not"
    print(f"k{k} r{r} step {step}: spans of {W} windows, K {K}, R {R}, L {L}, {nb} spans, loss {loss:g}, "
          f"{args.repeats} interleaved repeats")
    print(f"  lost symbols {lost}; recovered: windows {n_win} ({100 * n_win / lost:.2f} %), span {n_span} "
          f"({100 * n_span / lost:.2f} %); spans recovered {int((st == BLOCK_RECOVERED).sum())}")
    print(f"  span plan kernel     {med_range(t['plan'])}")
    print(f"  rows the compacted pass lists: {share:.3f} of K per tile of 16 unknowns ({tiles} tiles)")
    print(f"  span plan + apply, span_compact 0   {med_range(t['span0'])}")
    print(f"  span plan + apply, span_compact 1   {med_range(t['span'])}   {statistics.median(t['span']) / max(n_span, 1):.4f} us per recovered symbol")
    print(f"  row form, span_compact 0            {med_range(t['rows0'])}")
    print(f"  row form, span_compact 1            {med_range(t['rows1'])}   {statistics.median(t['rows1']) / max(n_span, 1):.4f} us per recovered symbol")
    print(f"  windows ({nw} blocks) {med_range(t['windows'])}   {statistics.median(t['windows']) / max(n_win, 1):.4f} us per recovered symbol",
          flush=True)


nspans = (1 << 16) // (16 if args.small else 1)
for loss in args.loss:
    for shape in ((30, 1, 5), (30, 5, 25), (32, 8, 8)):
        workload(*shape, 1200, nspans, loss)
        torch.cuda.empty_cache()
