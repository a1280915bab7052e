#!/usr/bin/env python3
"""What the Gauss-Newton tracker costs and what it buys, on the GPU.  Three sections, one JSON line each record:

  kernels    device time of mgs_pose_jacobian (its two launches, the tangent records and the tangent blend, together: the library
             has no switch between them), mgs_gn_normal_equations and mgs_pose_gn_step on a room map at 640 x 480 and at 1200 x 680, beside the blend forward's
             own stage time on the same lists and a device copy of the 30 planes' bytes.  Eager: every call timed on its own with a
             pair of device events, the variants alternating call by call, median of --calls (min, max beside it).  Replayed: the
             same call captured --inner times into one hipGraph, the replay's time divided by --inner.
  iteration  one captured Gauss-Newton iteration (GaussNewtonGraph) beside one captured Adam iteration (TrackingGraph): replays timed
             alternately on the same frame and map.
  slam       run_slam as `tools/slam_bench.py --config tum --room --graph` runs it, with tracker="adam" and "gauss_newton" alternated
             --rounds times: tracked frames per second, iterations per frame, ATE.

    python tools/gn_tracking_bench.py [--calls 30] [--warmup 5] [--inner 10] [--rounds 2] [--sections kernels,iteration,slam]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def room_map(intrinsics, iters=80):
    """(frames, intr, gmap, bg): a room map from its first keyframe, mapped for a few iterations, and a second frame to track."""
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.sequences import make_room_sequence
    frames, intr = make_room_sequence(2, intrinsics, device=DEV)
    vp = frames[0]
    vp.update_RT(vp.R_gt.clone(), vp.T_gt.clone())
    bg = torch.zeros(3, device=DEV)
    gmap = GaussianMap(DEV)
    gmap.extend_from_frame(vp, intr, downsample=8, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([vp], iters=iters, init=True)
    for p in gmap.params():
        p.grad = None
    return frames, intr, gmap, bg


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def kernels_section(args):
    from monogs_amd import _lib
    from monogs_amd.frames import Viewpoint
    from monogs_amd.pose_jacobian import NormalEquations, normal_equations
    from monogs_amd.pose_optim import PoseGaussNewton
    from monogs_amd.rasterizer import _stream, collect_timing, forward_scratch
    from monogs_amd.renderer import render
    lib = _lib.load()
    for name in ("fr3_office", "replica"):
        frames, intr, gmap, bg = room_map(name)
        vp = frames[0]
        with torch.no_grad():
            frozen = [t.detach().clone() for t in (gmap.get_xyz, gmap.get_rotation, gmap.get_scaling, gmap.get_opacity, gmap.get_features)]
        pkg = render(vp, intr, *frozen, bg)
        color, depth, opacity = pkg["render"], pkg["depth"], pkg["opacity"]
        t = forward_scratch(color)
        means3D, _, _, _, sc_, rot_, _, radii, _, _ = color.grad_fn.saved_tensors
        H, W, P = t.H, t.W, t.P
        J = torch.empty(6, 5, H, W, device=DEV)
        J2 = torch.empty_like(J)
        tan = torch.empty(lib.mgs_pose_tangent_bytes(P), dtype=torch.uint8, device=DEV)
        system = NormalEquations(torch.zeros(75, dtype=torch.float64, device=DEV))
        dummy = Viewpoint(-1, vp.rgb, vp.depth, DEV, grad_mask=vp.grad_mask)
        dummy.update_RT(vp.R.clone(), vp.T.clone())
        opt = PoseGaussNewton(dummy, max_rot=1e-6, max_trans=1e-6)          # (a step that barely moves: the time does not depend on it)

        def jac():
            _lib.check(lib.mgs_pose_jacobian(C.byref(t.cam), P, t.num_rendered, means3D.data_ptr(), sc_.data_ptr(), rot_.data_ptr(), None,
                                             radii.data_ptr(), *t.pointers(), tan.data_ptr(), J.data_ptr(), _stream()), "mgs_pose_jacobian")

        variants = {"pose_jacobian": jac,
                    "normal_equations": lambda: normal_equations(J, color, depth, opacity, vp, out=system),
                    "gn_step": lambda: opt.step_and_retract(system, sync=False),
                    "copy_30_planes": lambda: torch.add(J, 0.0, out=J2)}      # (a kernel: read + write of the planes' bytes, no memcpy node)
        jac()
        normal_equations(J, color, depth, opacity, vp, out=system)
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        eager, blend = {k: [] for k in variants}, []
        for _ in range(args.calls):
            for k, fn in variants.items():
                eager[k].append(timed(fn))
            with collect_timing() as sink, torch.no_grad():
                render(vp, intr, *frozen, bg)
            blend.append(sink[0]["blend_fwd_ms"])
        replayed = {}
        for k, fn in variants.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.inner):
                    fn()
            for _ in range(args.warmup):
                g.replay()
            torch.cuda.synchronize()
            replayed[k] = stats([timed(g.replay) / args.inner for _ in range(args.calls)])
        res = {"section": "kernels", "workload": f"room_{W}x{H}", "P": P, "num_rendered": t.num_rendered, "calls": args.calls,
               "inner": args.inner, "plane_bytes": 30 * H * W * 4, "blend_fwd": stats(blend),
               "eager": {k: stats(v) for k, v in eager.items()}, "replayed": replayed}
        print(json.dumps(res), flush=True)


def iteration_section(args):
    from monogs_amd.gn_tracking import GaussNewtonGraph
    from monogs_amd.tracking import TrackingGraph
    frames, intr, gmap, bg = room_map("fr3_office")
    vp = frames[1]
    vp.update_RT(frames[0].R_gt.clone(), frames[0].T_gt.clone())
    graphs = {"adam": TrackingGraph(vp, intr, gmap, bg), "gauss_newton": GaussNewtonGraph(vp, intr, gmap, bg)}
    times = {k: [] for k in graphs}
    for it in range(args.warmup + args.calls):
        for k, g in graphs.items():
            g._load(vp)                                   # a fresh, unconverged state: the replay does a whole iteration
            torch.cuda.synchronize()
            ms = timed(g.graphs[0].replay)
            if it >= args.warmup:
                times[k].append(ms)
    for g in graphs.values():
        g.close()
    res = {"section": "iteration", "workload": f"room_{intr.width}x{intr.height}", "P": len(gmap), "calls": args.calls}
    res.update({k: stats(v) for k, v in times.items()})
    res["gauss_newton_over_adam"] = round(res["gauss_newton"]["median_us"] / res["adam"]["median_us"], 2)
    print(json.dumps(res), flush=True)


def slam_section(args):
    from monogs_amd.slam_harness import run_slam
    cfg = dict(n_frames=args.frames, intrinsics="fr3_office", tracking_itr_num=100, mapping_itr_num=150, window_size=8, kf_interval=5,
               init_itr_num=300, scene="room", graph_tracking=True, graph_mapping=True)
    for rnd in range(args.rounds):
        for tracker in ("adam", "gauss_newton"):
            r = run_slam(tracker=tracker, **cfg)
            its = [n for _, n in r["track_iters_per_frame"]]
            print(json.dumps({"section": "slam", "round": rnd, "tracker": tracker, "frames": r["frames"], "width": r["width"],
                              "height": r["height"], "gaussians": r["gaussians"], "tracking_fps": round(r["tracking_fps"], 2),
                              "tracking_steady_iters_per_s": round(r["tracking_steady_iters_per_s"], 1),
                              "iters_per_frame_mean": round(sum(its) / len(its), 2), "iters_per_frame": its,
                              "ate_rmse_m": r["ate_rmse_m"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=11)
    ap.add_argument("--sections", default="kernels,iteration,slam")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gn_tracking_bench needs a GPU: there is no CPU path and no CPU number")
    for name in args.sections.split(","):
        {"kernels": kernels_section, "iteration": iteration_section, "slam": slam_section}[name](args)


if __name__ == "__main__":
    main()
