#!/usr/bin/env python3
"""Colour refinement (monogs_amd.refinement.Refiner) and render evaluation (monogs_amd.evaluation) against what a user
without them would run on the same GPU, at the TUM-like and Replica-like sizes of tools/slam_bench.py.

Refinement, iterations per second (wall clock around a synchronised run of --iters iterations, captures and capacity
measurements included): the captured loop, the eager loop, and the plain torch loop of tests/refinement_mirror.py (torch
activations, render() through the autograd seam, torch L1 + a two-pass conv2d SSIM on the GPU, torch.optim.Adam) -- all three
on the same map and keyframes.  Evaluation, device milliseconds per frame without the render: mgs_image_metrics +
mgs_ssim_forward against the torch composition (clamp, boolean-index PSNR, conv2d SSIM).  One process, the variants alternating
--alternations times; the spread is (max - min) / median over the repeats.  Prints one JSON line per size.

    python tools/refine_bench.py [--configs tum,replica] [--iters 200] [--alternations 3] [--gaussians 60000]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # refinement_mirror / mapping_mirror: the plain torch loop

CONFIGS = {"tum": "fr3_office", "replica": "replica"}
C1, C2 = 0.01 ** 2, 0.03 ** 2


def torch_ssim_valid(image, gt):
    """SSIM with padding "valid" composed in torch on the device: separable 11-tap Gaussian (zero padding), map cropped by 5."""
    k = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-k * k / 4.5)
    g = (g / g.sum()).float().to(image.device)
    C = image.shape[0]
    kh, kv = g.view(1, 1, 1, 11).repeat(C, 1, 1, 1), g.view(1, 1, 11, 1).repeat(C, 1, 1, 1)
    blur = lambda t: F.conv2d(F.conv2d(t, kh, padding=(0, 5), groups=C), kv, padding=(5, 0), groups=C)  # noqa: E731
    x, y = image[None], gt[None]
    mu1, mu2 = blur(x), blur(y)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return m[..., 5:-5, 5:-5].mean()


def torch_eval_frame(image, gt):
    """eval_rendering's per-frame arithmetic in torch ops, scalars left on the device."""
    c = torch.clamp(image, 0.0, 1.0)
    mask = gt > 0
    mse = ((c[mask] - gt[mask]) ** 2).mean()
    return 20 * torch.log10(1.0 / torch.sqrt(mse)), torch_ssim_valid(c, gt)


def stats(v, digits=2):
    s = sorted(v)
    med = s[len(s) // 2]
    return {"median": round(med, digits), "min": round(s[0], digits), "max": round(s[-1], digits),
            "spread": round((s[-1] - s[0]) / med, 4)}


def timed_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="tum,replica")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=60000)
    ap.add_argument("--keyframes", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refine_bench needs a GPU: there is no CPU path and no CPU number")
    from refinement_mirror import MirrorRefinement
    from monogs_amd.evaluation import _MetricsScratch, image_metrics
    from monogs_amd.gaussian_map import GaussianMap, REFERENCE_LR_SCHEDULE
    from monogs_amd.refinement import Refiner
    from monogs_amd.renderer import render
    from monogs_amd.slam_harness import make_sequence
    dev = "cuda:0"
    for name in args.configs.split(","):
        frames, intr = make_sequence(args.keyframes, CONFIGS[name], n_gaussians=args.gaussians, device=dev)
        for f in frames:
            f.update_RT(f.R_gt.clone(), f.T_gt.clone())
        bg = torch.zeros(3, device=dev)
        gmap = GaussianMap(dev)
        gmap.lr_schedule = dict(REFERENCE_LR_SCHEDULE, lr_init=gmap.lrs[0], lr_final=gmap.lrs[0] * 1e-2)
        gmap.extend_from_frame(frames[0], intr, downsample=8, init=True, point_size=1.0)
        eager, graph = Refiner(gmap, intr, bg, use_graph=False), Refiner(gmap, intr, bg, use_graph=True)
        mirror = MirrorRefinement(intr, bg, lr_schedule=gmap.lr_schedule, ssim=torch_ssim_valid)
        seq = Refiner.draw_sequence(len(frames), args.iters, 0)

        def run_mirror():
            opt = gmap.optimizer
            mirror.load_map(gmap.params(), opt.exp_avg, opt.exp_avg_sq, opt.t_dev.tolist(), opt.lrs, gmap.xyz_gradient_accum, gmap.denom,
                            gmap.max_radii_2d, gmap.kf_idx, gmap.nr_obs)
            mirror.load_keyframes(frames)
            mirror.iteration = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in seq:
                mirror.iterate(k)
            torch.cuda.synchronize()
            return args.iters / (time.perf_counter() - t0)

        def run_refiner(r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.refine(frames, args.iters)
            torch.cuda.synchronize()
            return args.iters / (time.perf_counter() - t0)

        run_refiner(eager); run_refiner(graph); run_mirror()                 # warm-up of everything the windows use
        rates = dict(graph=[], eager=[], torch_mirror=[])
        for _ in range(args.alternations):
            rates["graph"].append(run_refiner(graph))
            rates["eager"].append(run_refiner(eager))
            rates["torch_mirror"].append(run_mirror())
        graph.close(); eager.close()

        # evaluation: the per-frame arithmetic on one render, fused against the torch composition
        with torch.no_grad():
            image = render(frames[-1], intr, gmap.get_xyz, gmap.get_rotation, gmap.get_scaling, gmap.get_opacity, gmap.get_features,
                           bg)["render"].clone()
            gt = frames[-1].rgb
            H, W = int(intr.height), int(intr.width)
            row, clamped, sc = torch.empty(4, device=dev), torch.empty_like(image), _MetricsScratch(W, H, dev)
            ours = lambda: image_metrics(image, gt, row=row, clamped_out=clamped, scratch=sc)  # noqa: E731
            theirs = lambda: torch_eval_frame(image, gt)  # noqa: E731
            for _ in range(10):
                ours(); theirs()
            p, s = theirs()
            same = (abs(float(row[0]) - float(p)), abs(float(row[1]) - float(s)))
            t_ours, t_theirs = [], []
            for _ in range(args.alternations):
                t_ours.append(timed_ms(ours, 200))
                t_theirs.append(timed_ms(theirs, 200))
        so, st = stats(t_ours, 4), stats(t_theirs, 4)
        out = dict(config=name, width=W, height=H, gaussians=len(gmap), keyframes=len(frames), iters=args.iters,
                   refinement_it_per_s={k: stats(v, 1) for k, v in rates.items()},
                   graph_over_eager=round(stats(rates["graph"])["median"] / stats(rates["eager"])["median"], 2),
                   graph_over_torch_mirror=round(stats(rates["graph"])["median"] / stats(rates["torch_mirror"])["median"], 2),
                   refiner_stats=dict(graph=graph.stats, eager=eager.stats),
                   eval_ms_per_frame=dict(fused=so, torch=st, ratio_torch_over_fused=round(st["median"] / so["median"], 2),
                                          faster_beyond_spread=so["max"] < st["min"],
                                          psnr_abs_diff=same[0], ssim_abs_diff=same[1]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
