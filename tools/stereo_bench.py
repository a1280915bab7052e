#!/usr/bin/env python3
"""Device time per stereo pair of ``mgs_stereo_depth`` (monogs_amd.stereo.StereoMatcher.compute: twelve launches) at the EuRoC
size, 752 x 480 with 64 disparities and block 20 -- the reference's matcher -- with and without the rectification maps, and of
the whole ``StereoIngest.prepare_device`` (plus the eight launches of the gradient mask).

Every call is timed on its own with a pair of device events, after --warmup calls of each variant; the variants alternate call by
call inside one process and the figure is the median of --calls calls (min and max beside it).  The uploads are not in the
window.  ``*_replayed`` is the same call replayed from a captured graph.  Then, with the timing done: the launch count (the nodes
of the captured graph), the per-kernel device times of --trace-calls calls as the profiler lists them (median per kernel name),
and the bytes each stage has to move -- computed from the shapes, below -- against a device-to-device copy of the same order
measured in the same run.  Prints one JSON line per block of figures.

    python tools/stereo_bench.py [--size 752x480] [--disparities 64] [--block 20] [--calls 100] [--warmup 10]"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ingest_bench import capture, counted, graph_nodes, stats      # noqa: E402


def stage_bytes(W, H, D, maps):
    """Bytes each stage reads + writes when every operand crosses the memory interface once: what the layout costs, not what
    the caches save."""
    HW, HW1 = W * H, (W - D) * H
    vol = HW1 * D
    return {
        "stereo_prepare": 2 * HW + (16 * HW if maps else 0) + 2 * HW + 12 * HW,
        "stereo_prefilter": 2 * HW + 16 * HW,
        "stereo_hsum": 16 * HW + 2 * vol,
        "stereo_vsum": 2 * vol + 4 * vol,
        "stereo_path": (4 * vol + 4 * vol) + 4 * (8 * vol + 4 * vol),          # all five directions
        "stereo_winner": 4 * vol + 8 * HW1,
        "stereo_table": 6 * HW1 + 2 * HW,
        "stereo_finish": 2 * HW1 + 2 * HW + 6 * HW,
    }


def pair(W, H, seed=1):
    """A textured scene seen with a disparity that grows from 4 at the top to 40 at the bottom, sensor noise on both views."""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H, W + 64)).astype(np.float64)
    for _ in range(2):
        tex = (tex + np.roll(tex, 1, axis=1) + np.roll(tex, 1, axis=0) + np.roll(tex, -1, axis=1)) / 4.0
    tex = (tex - tex.min()) / (tex.max() - tex.min()) * 255.0
    disp = (4 + 36 * np.arange(H) / max(H - 1, 1)).astype(np.int64)
    left = np.stack([tex[y, 64 - disp[y]:64 - disp[y] + W] for y in range(H)])
    right = tex[:, 64:64 + W]
    noisy = lambda a: (a + rng.normal(0, 1.5, a.shape)).clip(0, 255).astype(np.uint8)      # noqa: E731
    return noisy(left), noisy(right)


def timed(fns, calls, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    return {k: stats(v) for k, v in times.items()}


def kernel_times(fn, calls):
    """Median device time per kernel name over ``calls`` calls, in microseconds, and how many launches of it one call makes."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    per = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            name = re.sub(r"^void\s+", "", e.name)
            name = re.sub(r"^mgs::", "", name)
            name = re.sub(r"\(.*$", "", name)
            per.setdefault(name, []).append(e.time_range.elapsed_us())
    return {k: {"median_us": round(sorted(v)[len(v) // 2], 1), "per_call": round(len(v) / calls, 2),
                "sum_per_call_us": round(sum(v) / calls, 1)} for k, v in sorted(per.items())}


def copy_ceiling(n_bytes, calls=20):
    """GB/s (read + write) of a device-to-device copy of ``n_bytes``: the ceiling the streaming stages are held against."""
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    t = []
    for _ in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        b.copy_(a)
        stop.record()
        stop.synchronize()
        t.append(start.elapsed_time(stop))
    ms = sorted(t)[len(t) // 2]
    return 2 * n_bytes / (ms * 1e-3) / 1e9, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="752x480")
    ap.add_argument("--disparities", type=int, default=64)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trace-calls", type=int, default=10)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stereo_bench needs a GPU: there is no CPU path and no CPU number")
    if args.calls < 50:
        sys.exit("--calls must be at least 50")
    from monogs_amd.stereo import StereoIngest, StereoMatcher, calibration_maps
    dev = "cuda:0"
    W, H = (int(v) for v in args.size.split("x"))
    D = args.disparities
    cal = json.load(open(os.path.join(ROOT, "tests", "golden", "euroc_calibration.json")))["Calibration"]
    s = W / 752.0
    for cam in ("cam0", "cam1"):
        for which in ("raw", "opt"):
            for k in ("fx", "fy", "cx", "cy"):
                cal[cam][which][k] *= s
    cal["width"], cal["height"] = W, H
    left, right = (torch.from_numpy(a).to(dev) for a in pair(W, H))
    maps = tuple(torch.from_numpy(m).to(dev) for m in calibration_maps(cal))
    kw = dict(num_disparities=D, block_size=args.block, uniqueness_ratio=40)
    matcher = StereoMatcher(W, H, dev, **kw)
    ingest = StereoIngest(W, H, cal, dev, **kw)
    variants = {"stereo": lambda: matcher.compute(left, right),
                "stereo_rectified": lambda: matcher.compute(left, right, maps),
                "ingest_rectified": lambda: ingest.prepare_device(left, right)}
    disp16 = variants["stereo"]()[0]
    torch.cuda.synchronize()
    valid = float((disp16[:, D:] >= 0).float().mean())
    out = {"width": W, "height": H, "num_disparities": D, "block_size": args.block, "calls": args.calls, "warmup": args.warmup,
           "valid_fraction": round(valid, 3), "scratch_bytes": matcher.scratch_bytes()}
    out.update(timed(variants, args.calls, args.warmup))
    graphs = {k: capture(fn)[0] for k, fn in variants.items()}
    out.update({k + "_replayed": v for k, v in timed({k: g.replay for k, g in graphs.items()}, args.calls, args.warmup).items()})
    out["frame_budget_us"] = 50000.0                      # EuRoC cameras deliver 20 frames per second
    print(json.dumps(out), flush=True)
    print(json.dumps({"launches": {k: counted(graph_nodes, fn) for k, fn in variants.items()}}), flush=True)
    need = stage_bytes(W, H, D, maps=False)
    gbs, ms = copy_ceiling(4 * (W - D) * H * D)
    traffic = {"copy_ceiling_GBps": round(gbs, 1), "copy_bytes": 8 * (W - D) * H * D, "copy_ms": round(ms, 4),
               "stage_bytes": need, "total_bytes": sum(need.values())}
    if not args.no_trace:
        try:
            per = kernel_times(variants["stereo"], args.trace_calls)
            traffic["kernels"] = per
            for stage, b in need.items():
                us = sum(v["sum_per_call_us"] for k, v in per.items() if stage in k)
                if us > 0:
                    traffic.setdefault("stage_GBps", {})[stage] = round(b / (us * 1e-6) / 1e9, 1)
                    traffic.setdefault("stage_us", {})[stage] = round(us, 1)
        except Exception as e:                                                           # noqa: BLE001
            traffic["kernels"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    print(json.dumps(traffic), flush=True)


if __name__ == "__main__":
    main()
