"""Idle latency of the synchronous hooks (tools/batch_load.c bl_hook_latency_mode): one block per call through
pquic_fec_{rlc,xor}_generate_repair_symbols / _recover, 2000 timed calls per direction after a warm-up.

Legs (name: scheme, shape, where the symbols lie, hook mode):
  rlc_staged         RLC k16 r4 L1200 e4, heap, staged        -- bench.py's hook leg, the default
  rlc_arena_staged   the same with the symbols in a registered arena, still staged (what the arena alone does)
  rlc_in_place       the same arena, pquic_fec_set_hooks_in_place(1): rows by address, no host copy
  xor_staged         XOR k4 r1 L1200, heap, staged            -- kernel launches and a stream synchronisation
  xor_worker_staged  XOR, heap, in-place mode: every row through a staging row, served by the resident worker
  xor_in_place       XOR, registered arena, in-place mode
One JSON line per leg: p50 / p99 / mean in us for generate and recover, recovered symbols per recover call,
and the in-place counters' movement (rows in place, rows staged, calls served by the worker, calls launched).

  python tools/hook_latency.py [--legs a,b,...] [--calls N] [--lib PATH/libbatchload.so]

--lib runs a load generator linked against another engine build (an A/B baseline); legs that build lacks
print {"leg": ..., "rc": -1}."""
import argparse
import ctypes as C
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# leg: (xor, k, r, L, e, arena, in_place)
LEGS = {
    "rlc_staged": (0, 16, 4, 1200, 4, 0, 0),
    "rlc_arena_staged": (0, 16, 4, 1200, 4, 1, 0),
    "rlc_in_place": (0, 16, 4, 1200, 4, 1, 1),
    "xor_staged": (1, 4, 1, 1200, 1, 0, 0),
    "xor_worker_staged": (1, 4, 1, 1200, 1, 0, 1),
    "xor_in_place": (1, 4, 1, 1200, 1, 1, 1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--lib", default=os.path.join(HERE, "libbatchload.so"))
    a = ap.parse_args()
    lib = C.CDLL(a.lib)
    D = C.POINTER(C.c_double)
    lib.bl_hook_latency_mode.argtypes = [C.c_int] * 6 + [C.c_long, C.c_int, C.c_int, D, C.POINTER(C.c_uint64)]
    for leg in a.legs.split(","):
        xor, k, r, L, e, arena, in_place = LEGS[leg]
        out = (C.c_double * 7)()
        rows = (C.c_uint64 * 4)()
        rc = lib.bl_hook_latency_mode(0, xor, k, r, L, e, a.calls, arena, in_place, out, rows)
        if rc:
            print(json.dumps({"leg": leg, "rc": rc}), flush=True)
            continue
        print(json.dumps({"leg": leg, "rc": 0, "k": k, "r": r, "L": L, "calls": a.calls,
                          "generate_us": {"p50": out[0], "p99": out[1], "mean": round(out[2], 2)},
                          "recover_us": {"p50": out[3], "p99": out[4], "mean": round(out[5], 2)},
                          "recovered_per_call": out[6], "rows": list(rows)}), flush=True)


if __name__ == "__main__":
    main()
