#!/usr/bin/env python3
"""Device time of the fused label loss (``label_loss_grads``: mgs_label_loss_grads, two launches) and of one
``ObjectLayerTrainer`` step at 640 x 480 and 1200 x 680 for K in {18, 64}, beside two comparisons taken in the same process:

  (a) ``torch_ce``: ``F.cross_entropy`` forward + backward on the same image and ids (``ignore_index`` for the ids the loss has
      no channel for): what a user composes without the label kernel;
  (b) ``copy``: a device copy that moves the loss's algorithmic bytes -- feat read once, d_feat written once, K H W floats each
      (ids and the count are a per cent of that): the memory floor of the same traffic.

The trainer step runs on a room map at the same size (one ray-cast keyframe back-projected and mapped for a few iterations): one
rasteriser forward, the feature forward, the loss, the feature backward, Adam on the rows.

Every call is timed on its own with a pair of device events, after --warmup calls of each variant; the variants alternate call
by call and the figure is the median of --calls calls (min and max beside it).  Prints one JSON line per (size, K).

    python tools/object_bench.py [--ks 18,64] [--calls 50] [--warmup 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"640x480": "fr3_office", "1200x680": "replica"}


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def room_map(intrinsics, K, dev):
    """(gmap, vp, intr, bg): a room map with K learned object rows seen from its keyframe; ids are the room's surface ids."""
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.sequences import make_room_sequence
    frames, intr = make_room_sequence(1, intrinsics, device=dev, with_segmentation=True)
    vp = frames[0]
    vp.update_RT(vp.R_gt.clone(), vp.T_gt.clone())
    bg = torch.zeros(3, device=dev)
    gmap = GaussianMap(dev, nr_objects=K, learn_objects=True)
    gmap.extend_from_frame(vp, intr, downsample=8, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([vp], iters=80, init=True)
    for p in gmap.params():
        p.grad = None
    return gmap, vp, intr, bg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="18,64")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("object_bench needs a GPU: there is no CPU path and no CPU number")
    import torch.nn.functional as F

    from monogs_amd.object_layer import LabelTarget, ObjectLayerTrainer, label_loss_grads, render_labels
    dev = "cuda:0"
    for size, intrinsics in SIZES.items():
        for K in (int(k) for k in args.ks.split(",")):
            gmap, vp, intr, bg = room_map(intrinsics, K, dev)
            H, W = int(intr.height), int(intr.width)
            feat, _ = render_labels(vp, intr, gmap, bg)                   # the image the loss sees in the trainer
            feat = feat.contiguous()
            target = LabelTarget(vp.segmentation)
            target.count(K)
            ids = vp.segmentation.long()
            tgt = torch.where(ids < K, ids, torch.full_like(ids, -100))[None]
            leaf = feat.clone()[None].requires_grad_(True)
            src, dst = torch.empty(K * H * W, device=dev), torch.empty(K * H * W, device=dev)
            trainer = ObjectLayerTrainer(gmap, intr, bg)

            def fused():
                return label_loss_grads(feat, target)

            def torch_ce():
                leaf.grad = None
                F.cross_entropy(leaf, tgt, ignore_index=-100).backward()
                return leaf.grad

            def copy():
                dst.copy_(src)

            def step():
                trainer.step(vp)

            variants = {"label_loss_grads": fused, "torch_ce": torch_ce, "copy": copy, "trainer_step": step}
            g = fused()
            agree = float((g.d_feat - torch_ce()[0]).abs().max())            # the timed variants compute the same thing
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
            nbytes = 2 * 4 * K * H * W
            res = {"size": size, "K": K, "P": len(gmap), "calls": args.calls, "warmup": args.warmup, "algorithmic_bytes": nbytes,
                   "max_abs_d_feat_vs_torch": agree, "counted_pixels": int(g.count)}
            for k in variants:
                res[k] = stats(times[k])
            res["label_loss_GBps"] = round(nbytes / (res["label_loss_grads"]["median_us"] * 1e-6) / 1e9, 1)
            res["copy_GBps"] = round(nbytes / (res["copy"]["median_us"] * 1e-6) / 1e9, 1)
            res["torch_ce_over_label_loss"] = round(res["torch_ce"]["median_us"] / res["label_loss_grads"]["median_us"], 2)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
