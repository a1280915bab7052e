#!/usr/bin/env python3
"""What the intrinsics gradient costs and what the calibration loop recovers (monogs_amd.calibration).

(a) Device time of the per-Gaussian backward (``mgs_timing.geom_bwd_ms`` of ``mgs_backward``: geom_backward_kernel + tau_finalize) with
    and without MGS_FLAG_INTRINSICS_GRAD, at C5 (2 M Gaussians, 1920x1080) and on a 40 k-Gaussian VGA map.  Without the flag the call
    launches the instantiations the parent commit launches (tools/kernel_identity.py: the same machine code), so the "off" column is
    the parent's figure for that kernel on this machine.  The two alternate --reps times in one process; median and spread.
(b) ``refine_intrinsics`` on the ray-cast room (``make_room_sequence``) at 160x120 and 640x480: a map back-projected from frame 0 at the
    true intrinsics and fitted to the three views for --map-iters iterations (monogs_amd.refinement.Refiner, still at the true
    intrinsics and poses), then frozen; start at fx x 1.04, fy x 0.97, cx + 3 and cy - 2 pixels per 160 pixels of width (PERTURBATION),
    default learning rates: iterations, final error per parameter, wall milliseconds per iteration.

One process under its own time limit (--time-limit seconds, SIGALRM ends it).  Prints one JSON line per measurement; nothing is asserted.

    python tools/calibration_bench.py [--reps 15] [--iters 80] [--map-iters 600] [--skip-c5] [--time-limit 540]"""
import argparse
import json
import os
import signal
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PERTURBATION = dict(fx=1.04, fy=0.97, cx=3.0 / 160, cy=-2.0 / 160)      # fx, fy: factors; cx, cy: shift as a fraction of the width


def stats(v, digits=4):
    s = sorted(v)
    med = s[len(s) // 2]
    return {"median": round(med, digits), "min": round(s[0], digits), "max": round(s[-1], digits),
            "spread": round((s[-1] - s[0]) / med, 4) if med else None}


def geom_backward_cost(P, intrinsics, reps, dev):
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, collect_timing
    from monogs_amd.synthetic import make_scene, scene_settings
    sc = make_scene(P, intrinsics, seed=2)
    st = scene_settings(sc, GaussianRasterizationSettings, device=dev)
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)  # noqa: E731
    xyz, rgb, opac, scaling, rot = leaf(sc.means3D), leaf(sc.colors), leaf(sc.opacities), leaf(sc.scales), leaf(sc.rotations)
    theta, rho = torch.zeros(3, device=dev, requires_grad=True), torch.zeros(3, device=dev, requires_grad=True)
    delta = torch.zeros(4, device=dev, requires_grad=True)
    g_color, g_depth = sc.grad_color.to(dev), sc.grad_depth.to(dev)
    rasterizer = GaussianRasterizer(st)

    def step(flag):
        for p in (xyz, rgb, opac, scaling, rot, theta, rho, delta):
            p.grad = None
        means2D = torch.zeros_like(xyz, requires_grad=True)
        color, _, depth, _, _ = rasterizer(means3D=xyz, means2D=means2D, opacities=opac, colors_precomp=rgb, scales=scaling,
                                           rotations=rot, theta=theta, rho=rho, intr=delta if flag else None)
        torch.autograd.backward([color, depth], [g_color, g_depth])

    for _ in range(3):
        step(False); step(True)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(reps):
        for flag in (False, True):
            with collect_timing() as sink:
                step(flag)
            ms[flag].append([d for d in sink if d["kind"] == "backward"][0]["geom_bwd_ms"])
    off, on = stats(ms[False]), stats(ms[True])
    return {"measurement": "geom_bwd_ms", "gaussians": P, "intrinsics": intrinsics, "reps": reps, "flag_off_ms": off, "flag_on_ms": on,
            "on_over_off": round(on["median"] / off["median"], 4), "dL_dk": [float(x) for x in delta.grad.tolist()]}


def room_recovery(scale, iters, map_iters, dev):
    from monogs_amd import camera as cam
    from monogs_amd.calibration import default_lrs, refine_intrinsics
    from monogs_amd.frames import Intrinsics
    from monogs_amd.gaussian_map import GaussianMap, REFERENCE_LR_SCHEDULE
    from monogs_amd.refinement import Refiner
    from monogs_amd.sequences import make_room_sequence
    k = dict(cam.INTRINSICS["fr3_office"])
    k = {n: (v // scale if n in ("W", "H") else v / scale) for n, v in k.items()}
    frames, true = make_room_sequence(3, k, device=dev, step_scale=8.0)
    for f in frames:
        f.update_RT(f.R_gt.clone(), f.T_gt.clone())
    gmap = GaussianMap(dev)
    gmap.lr_schedule = dict(REFERENCE_LR_SCHEDULE, lr_init=gmap.lrs[0], lr_final=gmap.lrs[0] * 1e-2)
    gmap.extend_from_frame(frames[0], true, downsample=max(8 // scale, 1), init=True, point_size=1.0)
    bg = torch.zeros(3, device=dev)
    refiner = Refiner(gmap, true, bg)
    fit = refiner.refine(frames, map_iters)
    refiner.close()
    start = dict(k, fx=k["fx"] * PERTURBATION["fx"], fy=k["fy"] * PERTURBATION["fy"], cx=k["cx"] + PERTURBATION["cx"] * k["W"],
                 cy=k["cy"] + PERTURBATION["cy"] * k["W"])
    intr = Intrinsics(start, dev, learnable=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    traj = refine_intrinsics(gmap, frames, intr, bg, iters=iters)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    names = ("fx", "fy", "cx", "cy")
    return {"measurement": "refine_intrinsics", "size": [k["W"], k["H"]], "gaussians": len(gmap), "views": len(frames), "map_iters": map_iters,
            "map_l1": [round(fit["first"]["l1"], 5), round(fit["last"]["l1"], 5)], "iters": iters,
            "lrs": list(default_lrs(intr)), "true": {n: k[n] for n in names}, "start": {n: round(start[n], 4) for n in names},
            "final": {n: round(traj["k"][-1][j], 4) for j, n in enumerate(names)},
            "final_error_px": {n: round(traj["k"][-1][j] - k[n], 4) for j, n in enumerate(names)},
            "loss": [round(traj["loss"][0], 5), round(traj["loss"][-1], 5)], "ms_per_iteration": round(ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--map-iters", type=int, default=600)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--time-limit", type=int, default=540)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calibration_bench needs a GPU: there is no CPU path and no CPU number")
    signal.alarm(args.time_limit)
    dev = "cuda:0"
    print(json.dumps(geom_backward_cost(40_000, "fr3_office", args.reps, dev)), flush=True)
    for scale in (4, 1):
        print(json.dumps(room_recovery(scale, args.iters, args.map_iters, dev)), flush=True)
    if not args.skip_c5:
        print(json.dumps(geom_backward_cost(2_000_000, "davis_1080p", args.reps, dev)), flush=True)


if __name__ == "__main__":
    main()
