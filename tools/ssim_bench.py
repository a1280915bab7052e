#!/usr/bin/env python3
"""Refinement loss (1 - lambda) L1 + lambda (1 - SSIM_valid): value + gradient, the fused HIP path against what a user without
the extension would run on the same GPU -- the torch composition of the same loss (two-pass grouped conv2d SSIM + L1,
autograd backward), float32.

One process, the two sides alternating; per side and size: warm-up, then windows of at least --window seconds timed with
device events, --alternations times; the spread is (max - min) / median over the repeats.  For ours also the time of the
forward (+ finalize) and of the backward on their own, the algorithmic bytes from the shapes (forward 8 + 12 bytes per value,
backward 12 + 8 read and 4 written) and the share of the 8 TB/s HBM peak.  Prints one JSON line per size.

    python tools/ssim_bench.py [--sizes 640x480,1200x680,1920x1080] [--window 0.5] [--alternations 3] [--once]

--once: one un-timed fused call per size and nothing else (for a kernel trace, `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12   # bytes / s
C1, C2 = 0.01 ** 2, 0.03 ** 2


def torch_refinement(image, gt, lam, g):
    """The same loss composed in torch: separable 11-tap Gaussian (zero padding), map cropped by 5, L1 mean."""
    C = image.shape[0]
    kh, kv = g.view(1, 1, 1, 11).repeat(C, 1, 1, 1), g.view(1, 1, 11, 1).repeat(C, 1, 1, 1)
    blur = lambda t: F.conv2d(F.conv2d(t, kh, padding=(0, 5), groups=C), kv, padding=(5, 0), groups=C)  # noqa: E731
    x, y = image[None], gt[None]
    mu1, mu2 = blur(x), blur(y)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return (1.0 - lam) * (image - gt).abs().mean() + lam * (1.0 - m[..., 5:-5, 5:-5].mean())


def timed_window(fn, seconds):
    """Mean device time per call (us) over a window of at least `seconds`."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total_ms, calls = 20, 0.0, 0
    while total_ms < seconds * 1e3:
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        total_ms += ms
        calls += n
        n = min(max(n, int(n * 0.25 * seconds * 1e3 / max(ms, 1e-3))), 100000)
    return total_ms * 1e3 / calls


def stats(v):
    s = sorted(v)
    med = s[len(s) // 2]
    return {"median_us": round(med, 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2),
            "spread": round((s[-1] - s[0]) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1200x680,1920x1080")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--lambda-ssim", type=float, default=0.2)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ssim_bench needs a GPU: there is no CPU path and no CPU number")
    from monogs_amd import _lib, fused_losses
    from monogs_amd.rasterizer import _stream
    lib = _lib.load()
    dev, lam = "cuda:0", args.lambda_ssim
    k = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-k * k / 4.5)
    g = (g / g.sum()).float().to(dev)
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        gen = torch.Generator().manual_seed(W * 31 + H)
        base = F.interpolate(torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=gen), size=(H, W), mode="bicubic")[0]
        image = (base + 0.05 * torch.randn(3, H, W, generator=gen)).clamp(0, 1).to(dev)
        gt = (base + 0.02 * torch.randn(3, H, W, generator=gen)).clamp(0, 1).to(dev)
        if args.once:
            rg = fused_losses.refinement_loss_grads(image, gt, lam)
            torch.cuda.synchronize()
            print(json.dumps({"size": size, "loss": float(rg.loss)}))
            continue
        leaf = image.clone().requires_grad_(True)

        def ours():
            fused_losses.refinement_loss_grads(image, gt, lam)

        def theirs():
            leaf.grad = None
            torch_refinement(leaf, gt, lam, g).backward()

        # the two halves of ours on their own, through the C ABI with buffers allocated once
        scratch = torch.empty(lib.mgs_ssim_scratch_bytes(3, W, H, 1) // 4, dtype=torch.float32, device=dev)
        d_render, loss = torch.empty_like(image), torch.empty((), dtype=torch.float32, device=dev)

        def fwd():
            _lib.check(lib.mgs_refine_loss_forward(W, H, lam, image.data_ptr(), gt.data_ptr(), scratch.data_ptr(), loss.data_ptr(),
                                                   _stream()), "mgs_refine_loss_forward")

        def bwd():
            _lib.check(lib.mgs_refine_loss_backward(W, H, lam, image.data_ptr(), gt.data_ptr(), scratch.data_ptr(), None,
                                                    d_render.data_ptr(), _stream()), "mgs_refine_loss_backward")

        for fn in (ours, theirs, fwd, bwd):                     # warm-up of every shape the windows use
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        # same numbers on both sides before anything is timed
        rg = fused_losses.refinement_loss_grads(image, gt, lam)
        theirs()
        rel = float((rg.d_render - leaf.grad).norm() / leaf.grad.norm())
        assert rel < 1e-3, rel
        t_ours, t_theirs, t_fwd, t_bwd = [], [], [], []
        for _ in range(args.alternations):
            t_ours.append(timed_window(ours, args.window))
            t_theirs.append(timed_window(theirs, args.window))
        for _ in range(args.alternations):
            t_fwd.append(timed_window(fwd, args.window / 2))
            t_bwd.append(timed_window(bwd, args.window / 2))
        so, st, sf, sb = stats(t_ours), stats(t_theirs), stats(t_fwd), stats(t_bwd)
        values = 3 * H * W
        b_fwd, b_bwd = values * (8 + 12), values * (12 + 8 + 4)
        out = {"size": size, "ours": so, "torch": st, "ratio_torch_over_ours": round(st["median_us"] / so["median_us"], 2),
               "faster_beyond_spread": so["max_us"] < st["min_us"],
               "gradient_rel_l2_ours_vs_torch": rel,
               "forward_plus_finalize": {**sf, "bytes": b_fwd, "hbm_share": round(b_fwd / (sf["median_us"] * 1e-6) / HBM_PEAK, 4)},
               "backward": {**sb, "bytes": b_bwd, "hbm_share": round(b_bwd / (sb["median_us"] * 1e-6) / HBM_PEAK, 4)}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
