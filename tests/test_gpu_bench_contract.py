"""`bench.py` prints ONE JSON line with the driver's contract fields (a small, fast configuration of the same code path)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_carries_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "3", "--no-slam",
                          "--no-cpu-baseline", "--gaussians", "200000", "--intrinsics", "fr3_office"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                      # ONE line on stdout; progress goes to stderr
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 3 and d["higher_is_better"] is True
    assert d["unit"] == "Mpix/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and d["config"]["workload"].startswith("custom")      # not the C5 configuration
    assert d["value"] > 0 and abs(d["value"] - 640 * 480 / 1e6 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1
    assert r["traffic"] is None                          # the stamped PMC files belong to the C5 workload only
    # the line says what ran BEFORE its timed region, without a look into `config`: the exact first step, the settle steps
    # (default 60, the first 20 of them timed as the cold figure) and the warm-up steps
    assert d["warmup_effective"] == 1 + d["config"]["settle_steps"] + (d["warmup"] - 1) == 63
    assert d["cold_steps"] == 20 and d["value_cold"] > 0
    assert abs(d["value_cold"] - 640 * 480 / 1e6 / (d["ms_per_step_cold"] * 1e-3)) < 0.01 * d["value_cold"]
    assert d["blend_in_timed_region"]["launches_timed"] <= 8       # the probes inside the timed region stay few


def _plain_run(out_dir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--gaussians", "200000",
                          "--intrinsics", "fr3_office", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """Without --full the line is the headline alone, --steps is the number of timed steps, and --dump-outputs writes what the
    last timed step returned (float32 / float64, <= 64 MB, per-Gaussian arrays at a seeded sample).  Two runs with the same arguments
    see the same inputs, so they write the same outputs (up to the order of the backward's atomic sums)."""
    d = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "Mpix/s" and d["dtype"] == "f32"
    assert abs(d["value"] - 640 * 480 / 1e6 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    for k in ("roofline", "cpu_baseline", "slam", "stages_ms", "value_cold", "blend_in_timed_region"):
        assert k not in d, k                       # measured behind --full only
    names = {"color", "depth", "opacity", "radii", "n_touched", "grad_means3D", "grad_means2D", "grad_opacities",
             "grad_colors_precomp", "grad_scales", "grad_rotations", "grad_theta", "grad_rho", "gaussian_index"}
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(a) == names
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["color"].shape == (3, 480, 640) and a["depth"].shape == (1, 480, 640)
    assert a["gaussian_index"].shape == (65536,) and a["grad_means3D"].shape == (65536, 3) and a["radii"].shape == (65536,)
    assert (a["radii"] > 0).any() and np.abs(a["grad_theta"]).max() > 0
    _plain_run(tmp_path / "b")
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    for k in ("color", "depth", "opacity", "radii", "n_touched", "gaussian_index"):
        assert np.array_equal(a[k], b[k]), k
    for k in names - {"color", "depth", "opacity", "radii", "n_touched", "gaussian_index"}:
        assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-5 * float(np.abs(b[k]).max())), k
