"""A benchmark probe: the tracking rate an UNMODIFIED MonoGS tracker gets from the drop-in, in five flavours from "only the
rasteriser swapped" to "everything fused" (``slam.eager_tracking`` in the bench line)."""
from __future__ import annotations

import time

import torch

from . import fused_losses
from .pose_optim import PoseAdam
from .renderer import render


def reference_style_tracking_loss(render_image, render_depth, render_opacity, viewpoint):
    """``get_loss_tracking`` in plain PyTorch ops, as the unmodified caller runs it (/root/reference/utils/slam_utils.py:58-98,
    ``invert_depth=False``): what an eager loop that swaps ONLY the rasteriser pays between the forward and the backward."""
    gt_depth = viewpoint.depth[None]
    opacity_mask = render_opacity > 0.99
    rgb = torch.exp(viewpoint.exposure_a) * render_image + viewpoint.exposure_b
    rgb_mask = viewpoint.mask * viewpoint.grad_mask * opacity_mask
    l1_rgb = (render_opacity * torch.abs(rgb * rgb_mask - viewpoint.rgb * rgb_mask).mean()).mean()
    depth_mask = (gt_depth > 0) * opacity_mask
    if depth_mask.any():
        l1_depth = torch.abs(render_depth[depth_mask] - gt_depth[depth_mask]).mean()
    else:
        l1_depth = torch.zeros((), device=render_depth.device)
    return 0.5 * l1_rgb + l1_depth


def eager_tracking_probe(frames, intr, gmap, bg, iters: int, profile_flavour=None):
    """The rate an UNMODIFIED MonoGS tracker gets from the drop-in: the loop of /root/reference/utils/slam_tracker.py:138-176
    -- ``render()`` through the seam (exact instance count: one read-back per forward, as upstream), the map's tensors
    requiring grad as the tracker's copy of the Gaussians does, ``loss.backward()``, ``torch.optim.Adam`` on the four pose /
    exposure parameters, ``update_pose`` -- with no hipGraph, no capacity mode.  Flavours, each a superset of the one before:
    ``torch_losses``      swaps ONLY the rasteriser: the loss is the reference's own torch ops (with their boolean-index
                          syncs), the pose step ``torch.optim.Adam`` + ``update_pose`` in torch ops (a host read-back each);
    ``fused_losses``      + ``monogs_amd.fused_losses.get_loss_tracking`` (same signature, two launches);
    ``fused_pose_step``   + ``PoseAdam.step_and_retract`` (Adam + retraction + camera tensors in one launch);
    ``render_loss_backward`` render + fused loss + backward, no pose step, with the device span of the same iterations;
    ``seam_only``         the same through the drop-in seam ALONE: the five map tensors handed over as already-activated
                          leaves, so that autograd stops at the rasteriser (no normalize / exp / sigmoid kernels and their
                          backward: those belong to the caller's GaussianModel getters) -- what tools/host_overhead.py times.
    Fixed iteration count (no early exit), pose and exposure restored afterwards."""
    import os
    from . import rasterizer as _r
    profile_flavour = profile_flavour or os.environ.get("MGS_PROBE_PROFILE")
    vp = frames[-1]
    keep = (vp.R.clone(), vp.T.clone(), vp.exposure_a.data.clone(), vp.exposure_b.data.clone())
    out = {}

    def map_tensors():
        return (gmap.get_xyz, gmap.get_rotation, gmap.get_scaling, gmap.get_opacity, gmap.get_features)

    def restore():
        with torch.no_grad():
            vp.update_RT(keep[0].clone(), keep[1].clone())
            vp.exposure_a.data.copy_(keep[2]); vp.exposure_b.data.copy_(keep[3])
            vp.cam_rot_delta.data.zero_(); vp.cam_trans_delta.data.zero_()
        for p in gmap.params():
            p.grad = None
    with _r.exact_counts():          # (the caller's mode and headroom are restored whatever happens inside)
        leaves = None
        for name in ("torch_losses", "fused_losses", "fused_pose_step", "render_loss_backward", "seam_only"):
            if name == "seam_only":
                with torch.no_grad():
                    leaves = [t.detach().clone().requires_grad_(True) for t in map_tensors()]
            loss_fn = reference_style_tracking_loss if name == "torch_losses" else fused_losses.get_loss_tracking
            if name in ("torch_losses", "fused_losses"):
                opt = torch.optim.Adam([dict(params=[vp.cam_rot_delta], lr=0.003), dict(params=[vp.cam_trans_delta], lr=0.001),
                                        dict(params=[vp.exposure_a], lr=0.01), dict(params=[vp.exposure_b], lr=0.01)])
                zero = opt.zero_grad
            else:
                popt = PoseAdam(vp, 0.003, 0.001, 0.01)
                zero = popt.zero_grad

            def it():
                zero()
                pkg = render(vp, intr, *(leaves if leaves is not None else map_tensors()), bg)
                loss = loss_fn(pkg["render"], pkg["depth"], pkg["opacity"], vp)
                loss.backward()
                if leaves is not None:
                    for t in leaves:
                        t.grad = None
                with torch.no_grad():
                    if name in ("torch_losses", "fused_losses"):
                        opt.step()
                        vp.retract()
                    elif name == "fused_pose_step":
                        popt.step_and_retract()
            # (un-timed iterations first, enough of them for the device to settle in the power state this loop keeps it in:
            #  behind a host-bound flavour it idles most of the time, and the first ~40 ms of load after that run slow)
            for _ in range(max(10, iters // 2)):
                it()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                it()
            e1.record()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[name] = dict(iters=iters, ms_per_iter=round(1e3 * dt / iters, 4), iters_per_s=round(iters / dt, 1))
            if profile_flavour == name:        # where the host time of this flavour goes (diagnostic)
                import cProfile
                import pstats
                import sys
                pr = cProfile.Profile()
                pr.enable()
                for _ in range(iters):
                    it()
                torch.cuda.synchronize()
                pr.disable()
                pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(18)
            restore()
        # device time of render + loss + backward alone: the same iteration with the host queued ahead (capacity mode)
        _r.set_sync_free(True)
        popt = PoseAdam(vp, 0.003, 0.001, 0.01)

        def it_dev():
            popt.zero_grad()
            pkg = render(vp, intr, *leaves, bg)
            fused_losses.get_loss_tracking(pkg["render"], pkg["depth"], pkg["opacity"], vp).backward()
            for t in leaves:
                t.grad = None
        for _ in range(max(10, iters // 2)):
            it_dev()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            it_dev()
        e1.record()
        torch.cuda.synchronize()
        out["seam_only"]["device_ms_per_iter"] = round(e0.elapsed_time(e1) / iters, 4)
        _r.set_sync_free(False)
        with _r.collect_timing() as sink:          # one exact iteration with HIP events between the stages: what the device does
            it_dev()
            torch.cuda.synchronize()
        st = {}
        for d in sink:
            st.update({k: round(v, 4) for k, v in d.items() if k.endswith("_ms") and v > 0})
            if d.get("kind") == "forward":
                out["seam_only"]["num_rendered"] = int(d["num_rendered"])
        out["seam_only"]["stages_ms"] = st
        _r.check_overflow()
        restore()
    out["gaussians"], out["width"], out["height"] = len(gmap), int(intr.width), int(intr.height)
    out["note"] = ("eager, exact instance count (one read-back per forward), map tensors require grad (ten-sum backward), fixed "
                   "iteration count against the final map of the run")
    return out
