#!/usr/bin/env python3
"""Device time per call of the monocular kernels beside their RGB-D neighbours, at the TUM and Replica sizes:

* ``fused_losses.loss_grads`` (``mgs_loss_grads``: forward + backward, two launches) in the tracking and the mapping flavour, RGB-D
  and ``rgb_only=True``, all four alternating call by call in one process;
* ``monocular.pseudo_depth`` (``mgs_pseudo_depth``) with a render (nine launches) and under the init rule (one), beside
  ``keyframe_window.masked_median`` on the same selection: the six of the nine launches that are the median's.

The method of tools/ingest_bench.py (its helpers are imported): every call timed on its own with a pair of device events after
--warmup calls of each variant, the median of --calls calls with min and max beside it, then the same calls replayed from a
captured graph (the device's share of the figure) and the graph's node counts.  Prints one JSON line per size.

    python tools/monocular_bench.py [--sizes 640x480,1200x680] [--calls 100] [--warmup 10]"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ingest_bench import capture, counted, graph_nodes, stats  # noqa: E402  (tools/ is the script directory)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1200x680")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("monocular_bench needs a GPU: there is no CPU path and no CPU number")
    from monogs_amd import fused_losses as F
    from monogs_amd.keyframe_window import masked_median
    from monogs_amd.monocular import pseudo_depth
    dev = "cuda:0"
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        U = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
        vp = types.SimpleNamespace(rgb=U(3, H, W), depth=1 + 3 * U(H, W), mask=U(H, W) > 0.05, grad_mask=U(H, W) > 0.4,
                                   exposure_a=torch.tensor([0.02], device=dev), exposure_b=torch.tensor([-0.01], device=dev))
        render, rdepth, opacity = U(3, H, W), 1 + 3 * U(1, H, W), 0.9 + 0.1 * U(1, H, W)
        noise, ok = torch.randn(H, W, device=dev, generator=g), U(H, W) > 0.02
        selected = torch.where((opacity[0] > 0.95) & ok, rdepth[0], torch.zeros_like(rdepth[0]))
        variants = {
            "tracking_rgbd": lambda: F.loss_grads(render, rdepth, opacity, vp, tracking=True),
            "tracking_rgb_only": lambda: F.loss_grads(render, None, opacity, vp, tracking=True, rgb_only=True),
            "mapping_rgbd": lambda: F.loss_grads(render, rdepth, None, vp, tracking=False),
            "mapping_rgb_only": lambda: F.loss_grads(render, None, None, vp, tracking=False, rgb_only=True),
            "pseudo_depth": lambda: pseudo_depth(rdepth, opacity, ok, noise=noise),
            "pseudo_depth_init": lambda: pseudo_depth(None, None, ok, noise=noise),
            "masked_median": lambda: masked_median(selected),
        }
        out = {"width": W, "height": H, "calls": args.calls, "warmup": args.warmup, "eager": timed(variants, args.calls, args.warmup)}
        graphs = {k: capture(fn) for k, fn in variants.items()}              # (the outputs stay alive with the graphs)
        out["replayed"] = timed({k: g_[0].replay for k, g_ in graphs.items()}, args.calls, args.warmup)
        out["launches"] = {k: counted(graph_nodes, fn) for k, fn in variants.items()}
        r = out["replayed"]
        out["rgb_only_over_rgbd"] = {k: round(r[k + "_rgb_only"]["median_us"] / r[k + "_rgbd"]["median_us"], 3)
                                     for k in ("tracking", "mapping")}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
