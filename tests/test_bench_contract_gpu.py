"""bench.py's one-line JSON contract on a real GPU (the driver parses this line every round): the
required keys and types, the roofline object consistent with itself, the CPU baseline's fields, and the
numbers sane -- on a short run of the default workload and of configs[3]."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _run(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def _check_common(d, steps, warmup, scaling="weak"):
    for key, typ in (("metric", str), ("value", (int, float)), ("unit", str), ("n_gpus", int), ("steps", int),
                     ("warmup", int), ("ms_per_step", (int, float)), ("higher_is_better", bool),
                     ("scaling", str), ("dtype", str), ("data", str), ("config", dict), ("roofline", dict)):
        assert isinstance(d.get(key), typ), (key, d.get(key))
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    # configs[3] splits a fixed 2^24 blocks over the GPUs (strong); the others fix the work per GPU
    assert d["higher_is_better"] is True and d["scaling"] == scaling and d["dtype"] == "u8"
    assert d["vs_baseline"] is None or isinstance(d["vs_baseline"], (int, float))
    assert d["value"] > 0 and d["ms_per_step"] > 0 and "workload" in d["config"]
    ro = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in ro, key
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0
    assert 0 < ro["achieved"] < ro["peak"]
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3
    assert ro["traffic"] is None or ro["traffic"] > 0


@pytest.mark.gpu
def test_bench_line_default_workload():
    d = _run(["--full", "--steps", "2", "--warmup", "1", "--no-legs", "--cpu-seconds", "1", "--cpu-blocks", "256"])
    _check_common(d, 2, 1)
    cpu = d["cpu_baseline"]
    assert isinstance(cpu, dict)
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cpu, key
    assert cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["kind"] in ("reference", "port")
    # the step's algorithmic rate cannot beat the dominant kernel's: value (GiB/s of k*L payload per step)
    # times (k + e) / k bytes per payload byte over two kernels is below the roofline kernel's rate
    assert d["value"] * 2 ** 30 / 1e9 < ro_rate(d)


def ro_rate(d):
    return d["roofline"]["achieved"]


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """A plain run (no --full): the line carries the headline fields and the step's own kernels, no CPU
    baseline and no side leg; --dump-outputs writes the last step's outputs as float32 .npy files, and they
    are the right bytes: the repairs equal the CPU oracle's for the sampled blocks, every recovered row
    equals the source it stands for."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from oracle_py import Oracle, synth_bytes
    nb, k, r, L = 2048, 16, 4, 1200
    d = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", str(nb), "--dump-outputs", str(tmp_path)])
    _check_common(d, 3, 1)
    assert d["cpu_baseline"] is None
    assert sorted(d["legs"]) == ["rlc_decode_k16_e4", "rlc_encode_k16_r4"]
    got = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert sorted(got) == ["recovered_mask", "recovered_rows", "repairs", "sample_blocks", "status"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = got["sample_blocks"].astype(np.int64)
    n = len(idx)
    assert n == min(nb, 1024) and np.all(np.diff(idx) > 0) and idx[-1] < nb
    assert got["repairs"].shape == (n, r, L) and got["recovered_rows"].shape == (n, r, L)
    assert got["status"].shape == (nb,) and got["recovered_mask"].shape == (n, 128)
    src = synth_bytes(nb * k * L, 0x5EEDF3C0).reshape(nb, k, L)
    assert np.array_equal(got["repairs"], Oracle().rlc_encode_batch(src, r, 0)[idx])
    ok = got["status"][idx] == 0
    assert ok.sum() >= 0.9 * n  # the rest: singular draws and the reference's own crash patterns
    mask = got["recovered_mask"][ok]
    assert np.all(mask.sum(1) == 4) and not mask[:, k:].any()
    lost = np.nonzero(mask)[1].reshape(-1, 4)  # ascending per block: the packed rows' order
    assert np.array_equal(got["recovered_rows"][ok], src[idx[ok, None], lost])


@pytest.mark.gpu
def test_bench_line_k32r8():
    d = _run(["--full", "--config", "k32r8", "--steps", "1", "--warmup", "1", "--no-cpu"])
    _check_common(d, 1, 1, scaling="strong")
    assert d["cpu_baseline"] is None
    assert "k32" in d["roofline"]["kernel"] or "<8," in d["roofline"]["kernel"]
    # the line printed only after the byte gate: every pass's sampled repairs decoded back to the sources
    g = d["config"]["encode_gate"]
    assert g["passes_checked"] == d["config"]["passes_per_step"] >= 1
    assert g["blocks_decoded_back"] >= 0.9 * 4096 * g["passes_checked"]
