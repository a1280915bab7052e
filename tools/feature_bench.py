#!/usr/bin/env python3
"""Device time of the K-channel feature forward and backward (mgs_features_forward / mgs_features_backward) for
K in {3, 8, 16, 32, 64} on two workloads at 640 x 480 -- a room map (one ray-cast keyframe back-projected and mapped for a few
iterations) and ``make_scene(100000, "fr3_office", seed=1)`` -- beside two comparisons taken in the same process:

  (a) ``blend_fwd``: the blend forward's own stage time on the same tables (mgs_timing.blend_fwd_ms of a forward of the same
      scene): what blending three colours, depth and opacity through these lists costs;
  (b) ``triples``: ceil(K / 3) complete ``GaussianRasterizer`` forwards with ``colors_precomp`` = a triple of feature columns,
      under ``torch.no_grad()``: what a user who wants a K-channel image has to run without the feature kernels.

Every call is timed on its own with a pair of device events, after --warmup calls of each variant; the variants alternate call
by call and the figure is the median of --calls calls (min and max beside it).  Prints one JSON line per (workload, K).

    python tools/feature_bench.py [--ks 3,8,16,32,64] [--calls 50] [--warmup 5]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def room_workload(dev):
    """(P, forward): a room map seen from its keyframe; ``forward(colors)`` renders it with the given [P,3] colours."""
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.renderer import render
    from monogs_amd.sequences import make_room_sequence
    frames, intr = make_room_sequence(1, "fr3_office", device=dev)
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
    return len(gmap), lambda colors: render(vp, intr, *frozen, colors, bg)["render"]


def scene_workload(dev):
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from monogs_amd.synthetic import make_scene, scene_settings
    sc = make_scene(100000, "fr3_office", seed=1)
    st = scene_settings(sc, GaussianRasterizationSettings, device=dev)
    means, opac, scales, rot = (t.to(dev) for t in (sc.means3D, sc.opacities, sc.scales.repeat(1, 3), sc.rotations))
    means2D = torch.zeros_like(means)
    return means.shape[0], lambda colors: GaussianRasterizer(st)(means3D=means, means2D=means2D, opacities=opac,
                                                                 colors_precomp=colors, scales=scales, rotations=rot)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="3,8,16,32,64")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feature_bench needs a GPU: there is no CPU path and no CPU number")
    from monogs_amd import _lib
    from monogs_amd.rasterizer import _stream, collect_timing, forward_scratch
    lib = _lib.load()
    dev = "cuda:0"
    for wname, make in (("room_640x480", room_workload), ("scene_100k_640x480", scene_workload)):
        P, forward = make(dev)
        g = torch.Generator().manual_seed(2)
        for K in (int(k) for k in args.ks.split(",")):
            feats = torch.rand(P, K, generator=g).to(dev)
            cols = torch.zeros(P, 3 * math.ceil(K / 3), device=dev)
            cols[:, :K] = feats
            triples = [cols[:, 3 * i:3 * i + 3].contiguous() for i in range(cols.shape[1] // 3)]
            color = forward(triples[0].clone().requires_grad_(True))       # the forward whose tables the feature kernels walk
            t = forward_scratch(color)
            H, W = t.H, t.W
            out = torch.empty(K, H, W, device=dev)
            d_out = (torch.rand(K, H, W, generator=g) / (H * W)).to(dev)
            d_feat = torch.empty(P, K, device=dev)
            scratch = t.pointers()

            def feat_fwd():
                _lib.check(lib.mgs_features_forward(C.byref(t.cam), P, K, t.num_rendered, *scratch, feats.data_ptr(), None,
                                                    out.data_ptr(), None, 0.5, _stream()), "mgs_features_forward")

            def feat_bwd():
                _lib.check(lib.mgs_features_backward(C.byref(t.cam), P, K, t.num_rendered, *scratch, d_out.data_ptr(),
                                                     d_feat.data_ptr(), _stream()), "mgs_features_backward")

            def triple_forwards():
                with torch.no_grad():
                    return [forward(c) for c in triples]

            variants = {"features_forward": feat_fwd, "features_backward": feat_bwd, "triples": triple_forwards}
            # the K-channel image both ways, once: the timed variants compute the same thing
            feat_fwd()
            ref = torch.cat(triple_forwards())[:K]
            agree = float((out - ref).abs().max())
            for _ in range(args.warmup):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            blend = []
            for _ in range(args.calls):
                for k, fn in variants.items():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    fn()
                    stop.record()
                    stop.synchronize()
                    times[k].append(start.elapsed_time(stop))
                with collect_timing() as sink, torch.no_grad():               # (a): the blend forward's stage time, same scene
                    forward(triples[0])
                blend.append(sink[0]["blend_fwd_ms"])
            res = {"workload": wname, "P": P, "K": K, "num_rendered": t.num_rendered, "calls": args.calls,
                   "warmup": args.warmup, "max_abs_vs_triples": agree, "blend_fwd": stats(blend),
                   "triple_forwards": len(triples)}
            for k in variants:
                res[k] = stats(times[k])
            res["triples_over_features_forward"] = round(res["triples"]["median_us"] / res["features_forward"]["median_us"], 2)
            res["features_forward_over_blend_fwd"] = round(res["features_forward"]["median_us"] / res["blend_fwd"]["median_us"], 2)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
