#!/usr/bin/env python3
"""Device time of a headless-viewer frame (monogs_amd.viewer) per mode, at the size and on the room map of
``tools/slam_bench.py --config tum --room`` (640 x 480, 11 frames), from the camera behind the last pose, with the keyframe
frustums, the trajectory and both current cameras drawn -- beside the plain no-grad rasteriser forward of the same map and camera,
taken in the same process.

Every variant is captured in a hipGraph once and replayed; each replay is timed on its own with a pair of device events after
--warmup replays, the variants alternate replay by replay, and the figure is the median of --calls replays (min and max beside
it).  ``launches`` is the number of kernels one frame runs (counted with the torch profiler on one eager frame; null where the
profiler reports none), ``us_per_launch`` the median divided by it.  Prints one JSON line per mode.

    python tools/viewer_bench.py [--frames 11] [--calls 40] [--warmup 5] [--out DIR]      # --out: also save one PNG per mode"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TUM = dict(intrinsics="fr3_office", tracking_itr_num=100, mapping_itr_num=150, window_size=8, kf_interval=5)     # slam_bench's "tum"


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:                     # (a profiler that cannot trace this device: the times stand without the count)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=11)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("viewer_bench needs a GPU: there is no CPU path and no CPU number")
    from monogs_amd import rasterizer as R
    from monogs_amd import viewer as V
    from monogs_amd.rasterizer import GaussianRasterizer
    from monogs_amd.renderer import raster_settings
    from monogs_amd.slam_harness import run_slam
    r = run_slam(n_frames=args.frames, init_itr_num=300, scene="room", nr_objects=18, graph_tracking=True, graph_mapping=True, **TUM)
    gmap, intr, frames = r["map"], r["intr"], r["frame_list"]
    kfs = [frames[i] for i in range(0, len(frames), TUM["kf_interval"])]
    snap = V.Snapshot.from_map(gmap, kfs, current=frames[-1], gt=frames[-1])
    bg = torch.zeros(3, device=snap.means.device)
    hv = V.HeadlessViewer(intr, bg)
    cam = V.view_behind(frames[-1], intr)
    rs = raster_settings(intr, bg, *cam.tensors(intr))
    P = len(gmap)
    m2d = torch.zeros_like(snap.means)

    def plain():
        with torch.no_grad():
            return GaussianRasterizer(rs)(means3D=snap.means, means2D=m2d, opacities=snap.opacity, colors_precomp=snap.features,
                                          scales=snap.scales, rotations=snap.rotations)[0]

    variants = {"forward_nograd": plain}
    for mode in V.MODES:
        variants[mode] = (lambda m: lambda: hv.frame(snap, cam, mode=m))(mode)
    R.check_overflow()
    launches, graphs, handle = {}, {}, R.graph_flags()
    for name, fn in variants.items():
        img = fn()                                          # eager: uploads the overlay, leaves the capacity hint
        if args.out and name in V.MODES:
            os.makedirs(args.out, exist_ok=True)
            V.save_png(img, os.path.join(args.out, f"{name}.png"))
        launches[name] = count_launches(fn)
        graphs[name] = torch.cuda.CUDAGraph()
        with handle, torch.cuda.graph(graphs[name]):
            fn()
    for _ in range(args.warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(args.calls):
        for k, g in graphs.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            g.replay()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    assert not R.check_overflow()
    handle.release()
    base = stats(times["forward_nograd"])
    for name in variants:
        res = dict(mode=name, P=P, width=int(intr.width), height=int(intr.height), segments=hv.overlay(snap, cam).S if name in V.MODES else 0,
                   calls=args.calls, warmup=args.warmup, launches=launches[name], **stats(times[name]))
        res["us_per_launch"] = round(res["median_us"] / launches[name], 2) if launches[name] else None
        res["over_forward_nograd"] = round(res["median_us"] / base["median_us"], 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
