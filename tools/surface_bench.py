#!/usr/bin/env python3
"""Device time of the surface kernels (mgs_surface_depth / mgs_depth_normals, csrc/surface.hip) on a room map -- one ray-cast
keyframe back-projected and mapped for a few iterations, as tools/feature_bench.py builds it -- at 640 x 480 (fr3_office) and at
1200 x 680 (replica), beside what they are to be set against, taken in the same process on the same tables:

  surface_median            mgs_surface_depth, MGS_SURFACE_MEDIAN alone (the early leave)
  surface_median_variance   mgs_surface_depth, both planes
  features_k3               mgs_features_forward at K = 3: a walk of the same lists that never leaves early
  copy_surface_planes       a device copy of the bytes the median + variance call writes (three [H, W] planes)
  depth_normals             mgs_depth_normals of the median depth
  copy_normals_bytes        a device copy of the bytes it reads and writes (one plane in, three out: the copy moves two planes each way)
  blend_fwd                 the blend forward's own stage time (mgs_timing.blend_fwd_ms of a forward of the same map)

Eagerly, every call is timed on its own with a pair of device events after --warmup calls of each variant; the variants alternate
call by call and the figure is the median of --calls calls (min and max beside it).  Replayed, every variant is captured into a graph
of --batch calls; the graphs alternate replay by replay and the figure is the median over --calls replays of the time per call.
Prints one JSON line per workload.

    python tools/surface_bench.py [--calls 50] [--warmup 5] [--batch 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def room_workload(dev, intrinsics):
    """(P, intr, forward): a room map seen from its keyframe; ``forward(colors)`` renders it with the given [P,3] colours."""
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.renderer import render
    from monogs_amd.sequences import make_room_sequence
    frames, intr = make_room_sequence(1, intrinsics, device=dev)
    vp = frames[0]
    vp.update_RT(vp.R_gt.clone(), vp.T_gt.clone())
    bg = torch.zeros(3, device=dev)
    gmap = GaussianMap(dev)
    gmap.extend_from_frame(vp, intr, downsample=8, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([vp], iters=80, init=True)
    with torch.no_grad():
        frozen = [t.detach().clone() for t in (gmap.get_xyz, gmap.get_rotation, gmap.get_scaling, gmap.get_opacity)]
        colors = gmap.get_features.detach().clone()
    return len(gmap), intr, colors, lambda c: render(vp, intr, *frozen, c, bg)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls per captured graph")
    ap.add_argument("--workloads", default="fr3_office,replica")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surface_bench needs a GPU: there is no CPU path and no CPU number")
    from monogs_amd import _lib
    from monogs_amd.rasterizer import _stream, collect_timing, forward_scratch
    lib = _lib.load()
    dev = "cuda:0"
    MED, VAR = _lib.H.MGS_SURFACE_MEDIAN, _lib.H.MGS_SURFACE_VARIANCE
    for intrinsics in args.workloads.split(","):
        P, intr, colors, forward = room_workload(dev, intrinsics)
        pkg = forward(colors.clone().requires_grad_(True))          # the forward whose tables the kernels walk
        t = forward_scratch(pkg["render"])
        H, W = t.H, t.W
        scratch = t.pointers()
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        median, variance, mid = f32(H, W), f32(H, W), torch.empty(H, W, dtype=torch.int32, device=dev)
        feat_out, normals = f32(3, H, W), f32(3, H, W)
        src3, dst3, src2, dst2 = f32(3, H, W).zero_(), f32(3, H, W), f32(2, H, W).zero_(), f32(2, H, W)
        fx, fy, cx, cy = (float(getattr(intr, k)) for k in ("fx", "fy", "cx", "cy"))

        def surface(want, max_std=0.0):
            _lib.check(lib.mgs_surface_depth(C.byref(t.cam), P, t.num_rendered, *scratch, want, 0.0, max_std, median.data_ptr(),
                                             mid.data_ptr(), variance.data_ptr(), _stream()), "mgs_surface_depth")

        def features_k3():
            _lib.check(lib.mgs_features_forward(C.byref(t.cam), P, 3, t.num_rendered, *scratch, colors.data_ptr(), None,
                                                feat_out.data_ptr(), None, 0.5, _stream()), "mgs_features_forward")

        def depth_normals():
            _lib.check(lib.mgs_depth_normals(W, H, median.data_ptr(), fx, fy, cx, cy, 0.05, normals.data_ptr(), _stream()),
                       "mgs_depth_normals")

        variants = {"surface_median": lambda: surface(MED), "surface_median_variance": lambda: surface(MED | VAR),
                    "features_k3": features_k3, "copy_surface_planes": lambda: dst3.copy_(src3),
                    "depth_normals": depth_normals, "copy_normals_bytes": lambda: dst2.copy_(src2)}
        # what the timed calls compute, once: the early leave changes nothing, the walk reproduces the forward's opacity split
        surface(MED | VAR)
        both = median.clone()
        surface(MED)
        opacity = pkg["opacity"].detach()[0]
        res = {"workload": f"room_{W}x{H}", "P": P, "num_rendered": t.num_rendered, "calls": args.calls, "warmup": args.warmup,
               "batch": args.batch, "median_alone_equals_median_with_variance": bool(torch.equal(both, median)),
               "pixels_with_median": int((mid >= 0).sum()), "pixels_opacity_ge_half": int((opacity >= 0.5).sum()),
               "mean_list_length": round(t.num_rendered / max(1, ((W + 15) // 16) * ((H + 15) // 16)), 1)}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times, blend = {k: [] for k in variants}, []
        for _ in range(args.calls):
            for k, fn in variants.items():
                times[k].append(timed(fn))
            with collect_timing() as sink, torch.no_grad():          # the blend forward's stage time, same map
                forward(colors)
            blend.append(sink[0]["blend_fwd_ms"])
        res["eager"] = {k: stats(v) for k, v in times.items()}
        res["eager"]["blend_fwd"] = stats(blend)
        # replayed: one graph of --batch calls per variant, the graphs alternating
        graphs = {}
        side = torch.cuda.Stream()
        for k, fn in variants.items():
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k], stream=side):
                for _ in range(args.batch):
                    fn()
        for _ in range(args.warmup):
            for g in graphs.values():
                g.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.calls):
            for k, g in graphs.items():
                times[k].append(timed(g.replay) / args.batch)
        res["replayed"] = {k: stats(v) for k, v in times.items()}
        for mode in ("eager", "replayed"):
            r = res[mode]
            r["median_over_features_k3"] = round(r["surface_median"]["median_us"] / r["features_k3"]["median_us"], 2)
            r["normals_over_copy"] = round(r["depth_normals"]["median_us"] / r["copy_normals_bytes"]["median_us"], 2)
        res["median_variance_over_blend_fwd"] = round(res["replayed"]["surface_median_variance"]["median_us"]
                                                      / res["eager"]["blend_fwd"]["median_us"], 2)
        print(json.dumps(res), flush=True)
        del graphs


if __name__ == "__main__":
    main()
