#!/usr/bin/env python3
"""Device time per frame of the frame ingest (monogs_amd.frame_ingest.FrameIngest.prepare_device: mgs_frame_prepare, nine
launches) at the TUM and Replica sizes, with and without the undistortion maps, beside the torch composition that does the
same work for the undistorted case on the same device inputs: ``/ 255``, permute, depth ``/ depth_scale``, a mask of ones and
``frames.scharr_grad_mask`` (pad, three convolutions, elementwise operations, ``torch.median``).

Every call is timed on its own with a pair of device events, after --warmup calls of each variant; the variants alternate call
by call inside one process and the figure is the median of --calls calls (min and max beside it).  The uploads are not in the
window: both paths need them.  ``*_replayed`` is the same call replayed from a captured graph.  Launch counts: the nodes of the
captured graph for the fused path, the profiler's device activities of one call for the torch composition (it cannot be captured:
it builds its filter taps with host-to-device copies).  Prints one JSON line per size, then one line of launch counts per size.

    python tools/ingest_bench.py [--sizes 640x480,1200x680] [--calls 100] [--warmup 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Dataset.Calibration of the TUM fr1_desk sequence (distorted), at 640 x 480; scaled with the width for other sizes
FR1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628,
           k3=1.163314, depth_scale=5000.0)


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def capture(fn, keep_graph=False):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def graph_nodes(fn):
    """Nodes of ``fn`` captured once in a graph: kernels and others (memset / memcpy)."""
    g, _ = capture(fn, keep_graph=True)
    hip = next(C.CDLL(ln.split()[-1]) for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    n = C.c_size_t(0)
    if hip.hipGraphGetNodes(C.c_void_p(g.raw_cuda_graph()), None, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (C.c_void_p * n.value)()
    hip.hipGraphGetNodes(C.c_void_p(g.raw_cuda_graph()), nodes, C.byref(n))
    kinds = []
    for node in nodes:
        t = C.c_int(-1)
        hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t))
        kinds.append(t.value)
    return {"how": "graph nodes", "kernels": kinds.count(0), "other": len(kinds) - kinds.count(0)}


def traced_launches(fn):
    """Device activities of one call of ``fn`` as the profiler lists them (for a variant that cannot be captured: the torch
    composition builds its filter taps with host-to-device copies)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = [n for n in names if n.lower().startswith(("memcpy", "memset", "copy"))]
    return {"how": "profiler trace", "kernels": len(names) - len(copies), "other": len(copies)}


def counted(how, fn):
    try:
        return how(fn)
    except Exception as e:                                                               # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"[:160]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1200x680")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-launch-counts", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ingest_bench needs a GPU: there is no CPU path and no CPU number")
    if args.calls < 50:
        sys.exit("--calls must be at least 50")
    from monogs_amd.frame_ingest import FrameIngest
    from monogs_amd.frames import scharr_grad_mask
    dev = "cuda:0"
    results = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        s = W / 640.0
        cal = dict(FR1, **{k: FR1[k] * s for k in ("fx", "fy", "cx", "cy")}, width=W, height=H)
        rng = np.random.default_rng(1)
        # a smooth image with noise on top, so that the gradient intensities are spread as a photograph's are
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 80 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + rng.normal(0, 12, (H, W, 3))
        rgb = torch.from_numpy(base.clip(0, 255).astype(np.uint8)).to(dev)
        depth = torch.from_numpy(rng.integers(2000, 30000, size=(H, W), dtype=np.uint16)).to(dev)
        depth_i32 = depth.to(torch.int32)                     # (torch has no arithmetic on uint16)
        plain = FrameIngest(W, H, dict(cal, distorted=False), dev)
        warped = FrameIngest(W, H, dict(cal, distorted=True), dev)

        def torch_path(rgb=rgb, depth_i32=depth_i32):           # (defaults: bound now, the loop goes on to the next size)
            image = (rgb / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).contiguous()
            d = depth_i32.to(torch.float32) / 5000.0
            return image, d, torch.ones_like(d, dtype=torch.bool), scharr_grad_mask(image)

        variants = {"fused": lambda fi=plain, rgb=rgb, depth=depth: fi.prepare_device(rgb, depth),
                    "fused_distorted": lambda fi=warped, rgb=rgb, depth=depth: fi.prepare_device(rgb, depth),
                    "torch": torch_path}
        a, b = variants["fused"](), variants["torch"]()
        torch.cuda.synchronize()
        agree = dict(rgb_max_abs=float((a["rgb"] - b[0]).abs().max()), depth_max_abs=float((a["depth"] - b[1]).abs().max()),
                     grad_mask_differs=int((a["grad_mask"] != b[3]).sum()))
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.calls):
            for k, fn in variants.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn()
                stop.record()
                stop.synchronize()
                times[k].append(start.elapsed_time(stop))
        out = {"width": W, "height": H, "calls": args.calls, "warmup": args.warmup, "fused_vs_torch": agree}
        for k in variants:
            out[k] = stats(times[k])
        out["torch_over_fused"] = round(out["torch"]["median_us"] / out["fused"]["median_us"], 2)
        # the same nine launches replayed from a captured graph: the device's share of the figures above
        graphs = {k: capture(variants[k])[0] for k in ("fused", "fused_distorted")}
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
        for k in graphs:
            out[k + "_replayed"] = stats(times[k])
        print(json.dumps(out), flush=True)
        results.append((size, variants))
    if not args.no_launch_counts:                # (after every timing: tracing slows the host)
        for size, variants in results:
            print(json.dumps({"size": size, "launches": {
                "fused": counted(graph_nodes, variants["fused"]), "fused_distorted": counted(graph_nodes, variants["fused_distorted"]),
                "torch": counted(traced_launches, variants["torch"])}}), flush=True)


if __name__ == "__main__":
    main()
