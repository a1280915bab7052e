#!/usr/bin/env python3
"""Device time of the rigid object transform (``mgs_object_transform_forward``: one launch; ``mgs_object_transform_backward``: two)
for P in {4 x 10^4, 2 x 10^6} Gaussians and M in {1, 16} moving objects, beside a device copy of the same bytes taken in the same
process, and of one ``ObjectTracker`` iteration beside one camera-tracking iteration on the same map.

Half of the Gaussians carry a moving id, spread evenly over the M objects, in random order: every wave of the backward meets every
slot (the worst case for its per-slot butterflies).  Bytes per Gaussian: forward 57 (label 1, mean 12 and quaternion 16 read, mean
and quaternion written), backward 85 (label, x', q', g, gq read, the two input gradients written); the copy moves the same number
of bytes (half read, half written).

  eager     every call launched from Python and timed on its own with a pair of device events: at the small size this is the
            launch path, not the kernels;
  replayed  --reps calls captured in ONE hipGraph; the time of a replay over --reps: the kernels back to back.
  ``copy`` is ``Tensor.copy_`` (eager only: a captured copy_ is a memcpy node, which the hot path avoids, csrc/common.h), ``copy_kernel``
  the same bytes through an elementwise kernel (``torch.mul(src, 1, out=dst)``), eager and replayed.

The variants alternate call by call; the figure is the median of --calls (min and max beside it).  One JSON line per (P, M), one
for the tracker.

    python tools/object_motion_bench.py [--sizes 40000,2000000] [--objects 1,16] [--calls 30] [--warmup 5] [--reps 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v, div=1):
    s = sorted(x / div for x in v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def run_variants(variants, calls, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(calls):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    return times


def captured(fn, reps):
    """``reps`` calls of ``fn`` in one graph (after a warm-up on a side stream, as torch asks); returns the replay function."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g.replay


def transform_case(P, M, args, dev):
    from monogs_amd import _lib
    from monogs_amd.object_motion import ObjectPoses
    from monogs_amd.rasterizer import _stream
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(P + M)
    poses = ObjectPoses(list(range(3, 3 + M)), dev)
    poses.R.copy_(torch.linalg.qr(torch.randn(M, 3, 3, device=dev, generator=gen))[0])
    poses.T.copy_(torch.randn(M, 3, device=dev, generator=gen))
    labels = torch.randint(0, 2 * M, (P,), device=dev, generator=gen).to(torch.uint8) + 3          # ids 3 .. 3 + 2M - 1: half of them move
    x, q = torch.randn(P, 3, device=dev, generator=gen), torch.nn.functional.normalize(torch.randn(P, 4, device=dev, generator=gen))
    gx, gq = torch.randn(P, 3, device=dev, generator=gen), torch.randn(P, 4, device=dev, generator=gen)
    xo, qo, dx, dq = torch.empty_like(x), torch.empty_like(q), torch.empty_like(x), torch.empty_like(q)
    tau = torch.empty(M, 6, device=dev)
    scratch = torch.empty(lib.mgs_object_motion_scratch_bytes(P, M), dtype=torch.uint8, device=dev)
    fwd_bytes, bwd_bytes = 57 * P, 85 * P
    src_f, dst_f = torch.empty(fwd_bytes // 8, device=dev), torch.empty(fwd_bytes // 8, device=dev)
    src_b, dst_b = torch.empty(bwd_bytes // 8, device=dev), torch.empty(bwd_bytes // 8, device=dev)
    tab = poses.slot_of_label.data_ptr()

    def forward():
        _lib.check(lib.mgs_object_transform_forward(P, M, labels.data_ptr(), tab, poses.R.data_ptr(), poses.T.data_ptr(), x.data_ptr(),
                                                    q.data_ptr(), xo.data_ptr(), qo.data_ptr(), _stream()), "forward")

    def backward():
        _lib.check(lib.mgs_object_transform_backward(P, M, labels.data_ptr(), tab, poses.R.data_ptr(), xo.data_ptr(), qo.data_ptr(),
                                                     gx.data_ptr(), gq.data_ptr(), dx.data_ptr(), dq.data_ptr(), tau.data_ptr(),
                                                     scratch.data_ptr(), _stream()), "backward")

    eager = {"forward": forward, "backward": backward, "copy_fwd_bytes": lambda: dst_f.copy_(src_f), "copy_bwd_bytes": lambda: dst_b.copy_(src_b),
             "copy_kernel_fwd_bytes": lambda: torch.mul(src_f, 1.0, out=dst_f), "copy_kernel_bwd_bytes": lambda: torch.mul(src_b, 1.0, out=dst_b)}
    forward()
    te = run_variants(eager, args.calls, args.warmup)
    replay = {k: captured(eager[k], args.reps) for k in ("forward", "backward", "copy_kernel_fwd_bytes", "copy_kernel_bwd_bytes")}
    tr = run_variants(replay, args.calls, args.warmup)
    res = {"P": P, "M": M, "moving": int((poses.slot_of_label[labels.long()] >= 0).sum()), "calls": args.calls, "reps": args.reps,
           "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes, "eager": {k: stats(v) for k, v in te.items()},
           "replayed": {k: stats(v, args.reps) for k, v in tr.items()}}
    r = res["replayed"]
    res["forward_GBps"] = round(fwd_bytes / (r["forward"]["median_us"] * 1e-6) / 1e9, 1)
    res["backward_GBps"] = round(bwd_bytes / (r["backward"]["median_us"] * 1e-6) / 1e9, 1)
    res["forward_over_copy"] = round(r["forward"]["median_us"] / r["copy_kernel_fwd_bytes"]["median_us"], 2)
    res["backward_over_copy"] = round(r["backward"]["median_us"] / r["copy_kernel_bwd_bytes"]["median_us"], 2)
    print(json.dumps(res), flush=True)


def tracker_case(args, dev):
    """One ``ObjectTracker`` iteration and one camera-tracking iteration (``track_eager``'s body, flag not read) on one map: the dynamic
    room at 640 x 480, a quarter of the pixels back-projected."""
    from monogs_amd import fused_losses
    from monogs_amd.frames import Viewpoint
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.map_step import render_map
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.object_motion import MovedMap, ObjectPoses, ObjectTracker
    from monogs_amd.pose_optim import PoseAdam
    from monogs_amd.sequences import DYNAMIC_BOX_ID, make_dynamic_room_sequence
    frames, intr, _ = make_dynamic_room_sequence(2, "fr3_office", dev)
    bg = torch.zeros(3, device=dev)
    gmap = GaussianMap(dev, nr_objects=DYNAMIC_BOX_ID + 1)
    frames[0].update_RT(frames[0].R_gt.clone(), frames[0].T_gt.clone())
    gmap.extend_from_frame(frames[0], intr, downsample=2, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([frames[0]], iters=80, init=True)
    for p in gmap.params():
        p.grad = None
    f = frames[1]
    vp = Viewpoint(f.frame_idx, f.rgb, f.depth, dev, gt_R=f.R_gt, gt_T=f.T_gt, segmentation=f.segmentation)
    vp.update_RT(f.R_gt.clone(), f.T_gt.clone())
    poses = ObjectPoses([DYNAMIC_BOX_ID], dev)
    tracker = ObjectTracker(intr, gmap, bg, poses)
    tracker.load(vp)
    opt = PoseAdam(vp, 0.003, 0.001, 0.01)
    cam_map = MovedMap(gmap, tracker.labels, ObjectPoses([], dev))     # nothing moves: the detached map the camera tracker renders

    def camera_iteration():
        pkg = render_map(vp, intr, cam_map, bg)
        opt.zero_grad()
        fused_losses.get_loss_tracking(pkg["render"], pkg["depth"], pkg["opacity"], vp).backward()
        opt.step_and_retract(sync=False)

    times = run_variants({"object_tracker_iteration": tracker.iteration, "camera_tracking_iteration": camera_iteration}, args.calls, args.warmup)
    res = {"size": "640x480", "P": len(gmap), "moving": int((tracker.labels == DYNAMIC_BOX_ID).sum()), "calls": args.calls}
    res.update({k: stats(v) for k, v in times.items()})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40000,2000000")
    ap.add_argument("--objects", default="1,16")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-tracker", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("object_motion_bench needs a GPU: there is no CPU path and no CPU number")
    dev = "cuda:0"
    for P in (int(v) for v in args.sizes.split(",")):
        for M in (int(v) for v in args.objects.split(",")):
            transform_case(P, M, args, dev)
    if not args.no_tracker:
        tracker_case(args, dev)


if __name__ == "__main__":
    main()
