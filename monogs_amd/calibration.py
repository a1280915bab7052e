"""Camera self-calibration: Adam on the four pinhole numbers (fx, fy, cx, cy) from the intrinsics gradient the rasteriser's backward
sums beside the pose gradient (``MGS_FLAG_INTRINSICS_GRAD``; DESIGN.md section 3, "Intrinsics gradient").

The reference keeps ``fx`` / ``fy`` as ``nn.Parameter``s with a TODO (/root/reference/utils/camera_utils.py:26-28) and ships guessed
intrinsics for its only 1080p config (configs/mono/davis/car-turn.yaml); its rasteriser gives the camera matrices no gradient, so it
has no learning rates to take over: the defaults below are this project's choice (DESIGN.md records the experiment behind them).

Eager only.  ``tanfovx`` / ``tanfovy`` are host scalars of ``mgs_camera``, so every step reads the new values back (16 bytes) to
rebuild the settings; intrinsics inside a captured iteration need them on the device and are out of scope.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, fused_losses
from .map_step import render_map
from .pose_optim import PoseAdam
from ._launch import _device_guard, _stream

NAMES = ("fx", "fy", "cx", "cy")
# Default learning rates, in pixels per step per pixel of image width (Adam's step is about one learning rate while the gradient
# keeps its sign), and the factor they decay to.  A choice -- the reference has none -- from the room experiment in DESIGN.md.
LR_FOCAL_PER_WIDTH, LR_CENTRE_PER_WIDTH, LR_FINAL = 2e-3, 1e-3, 0.01


def default_lrs(intr):
    """``(lr_focal, lr_centre)`` in pixels for the image width of ``intr``."""
    return LR_FOCAL_PER_WIDTH * float(intr.width), LR_CENTRE_PER_WIDTH * float(intr.width)


class IntrinsicsAdam:
    """Adam (torch.optim.Adam defaults) on ``intr``'s four numbers, ``intr`` a ``frames.Intrinsics(learnable=True)``.

    The parameters (a device copy of ``fx, fy, cx, cy``), both moments and the step counts live on the device.  ``step()`` runs ONE
    ``mgs_adam_step`` call over the focal pair (``lr_focal``) and the centre pair (``lr_centre``) on ``intr.delta.grad`` masked by
    ``free`` -- a component that is not free sees a zero gradient, so zero moments and no motion -- then makes ONE 16-byte
    read-back of the new values, calls ``intr.set(...)`` and zeroes the delta and its gradient.  That read-back is the price of
    ``tanfovx`` / ``tanfovy`` being host scalars in ``mgs_camera``: the next render needs them on the host.  The loop is therefore
    eager-only: ``step()`` raises under an active stream capture, before it launches anything."""

    def __init__(self, intr, lr_focal=None, lr_centre=None, free=NAMES, betas=(0.9, 0.999), eps=1e-8):
        if getattr(intr, "delta", None) is None:
            raise ValueError("IntrinsicsAdam needs learnable intrinsics: frames.Intrinsics(k, device, learnable=True)")
        unknown = [n for n in free if n not in NAMES]
        if unknown:
            raise ValueError(f"free: unknown parameter names {unknown}; choose from {NAMES}")
        self.intr, self.free = intr, tuple(free)
        d_focal, d_centre = default_lrs(intr)             # learning rates in pixels per step; None: default_lrs(intr)
        self.lrs = (float(d_focal if lr_focal is None else lr_focal), float(d_centre if lr_centre is None else lr_centre))
        self.betas, self.eps = betas, float(eps)
        dev = intr.delta.device
        self.k = torch.tensor([intr.fx, intr.fy, intr.cx, intr.cy], dtype=torch.float32, device=dev)
        self.m, self.v = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
        self.t_dev = torch.zeros(2, dtype=torch.int32, device=dev)            # one Adam step count per pair
        self.mask = torch.tensor([1.0 if n in self.free else 0.0 for n in NAMES], dtype=torch.float32, device=dev)

    def zero_grad(self):
        self.intr.delta.grad = None

    @torch.no_grad()
    def step(self, lr_scale: float = 1.0):
        """One Adam step from ``intr.delta.grad``, both learning rates times ``lr_scale`` (a schedule); returns the new
        ``(fx, fy, cx, cy)`` as Python floats."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("IntrinsicsAdam.step() is eager-only: the new intrinsics are read back to the host (tanfovx / tanfovy "
                               "are host scalars of mgs_camera), which a stream capture cannot record")
        grad = self.intr.delta.grad
        if grad is None:
            raise RuntimeError("IntrinsicsAdam.step(): intr.delta has no gradient; render with these intrinsics and back-propagate first")
        lib = _lib.load()
        g = grad.detach().to(torch.float32).contiguous() * self.mask
        pair = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr() + 8)  # noqa: E731   (focal pair, centre pair)
        with _device_guard(self.k.device):
            _lib.check(lib.mgs_adam_step(2, pair(self.k), pair(g), pair(self.m), pair(self.v), (C.c_uint64 * 2)(2, 2),
                                         (C.c_float * 2)(self.lrs[0] * lr_scale, self.lrs[1] * lr_scale), self.betas[0],
                                         self.betas[1], self.eps, 0,
                                         self.t_dev.data_ptr(), None, _stream()), "mgs_adam_step")
        fx, fy, cx, cy = self.k.tolist()                    # the ONE read-back (16 bytes) of the step
        self.intr.set(fx, fy, cx, cy)
        self.intr.delta.data.zero_()
        self.intr.delta.grad = None
        return fx, fy, cx, cy


def refine_intrinsics(gmap, viewpoints, intr, bg, iters: int, free=NAMES, poses: str = "fixed", lrs=None, lr_final: float = LR_FINAL):
    """Fit ``intr`` (``frames.Intrinsics(learnable=True)``) to ``viewpoints`` against the map ``gmap``, which is not changed (it is
    rendered detached).  Every iteration renders every viewpoint (``render_map``), sums ``fused_losses.get_loss_mapping`` -- the
    RGB-only mapping loss for a ``sensor="monocular"`` viewpoint -- runs one backward, steps ``IntrinsicsAdam`` and, with
    ``poses="free"``, one ``PoseAdam`` per viewpoint (the reference's pose learning rates).  ``lrs``: ``(lr_focal, lr_centre)``, by
    default the module's; they fall log-linearly to ``lr_final`` times their value over the ``iters`` iterations (the L1 losses do
    not flatten at the optimum, so a constant Adam step keeps hopping across it by about one learning rate).  Returns
    ``dict(k=[(fx, fy, cx, cy) before the first iteration and after each], loss=[the summed loss of each iteration])``; reading
    the loss synchronises once per iteration, as the intrinsics read-back does anyway."""
    if poses not in ("fixed", "free"):
        raise ValueError('poses must be "fixed" or "free"')
    lr_focal, lr_centre = default_lrs(intr) if lrs is None else lrs
    opt = IntrinsicsAdam(intr, lr_focal, lr_centre, free=free)
    pose_opts = [PoseAdam(vp) for vp in viewpoints] if poses == "free" else []
    frozen = _DetachedMap(gmap)
    traj_k, traj_loss = [(intr.fx, intr.fy, intr.cx, intr.cy)], []
    for it in range(int(iters)):
        opt.zero_grad()
        for vp in viewpoints:
            for p in (vp.cam_rot_delta, vp.cam_trans_delta, vp.exposure_a, vp.exposure_b):
                p.grad = None
        total = None
        for vp in viewpoints:
            pkg = render_map(vp, intr, frozen, bg)
            if getattr(vp, "sensor", "depth") == "monocular":
                loss = fused_losses.get_loss_mapping_rgb(pkg["render"], pkg["depth"], vp)
            else:
                loss = fused_losses.get_loss_mapping(pkg["render"], pkg["depth"], vp)
            total = loss if total is None else total + loss
        total.backward()
        traj_loss.append(float(total.item()))
        traj_k.append(opt.step(lr_scale=float(lr_final) ** (it / max(int(iters) - 1, 1))))
        for po in pose_opts:
            po.step_and_retract(sync=False)
    return dict(k=traj_k, loss=traj_loss)


class _DetachedMap:
    """What ``render_map`` reads of a ``GaussianMap``, detached: the renders of ``refine_intrinsics`` give the map no gradient."""
    fused_adam = False

    def __init__(self, gmap):
        with torch.no_grad():
            self.get_xyz, self.get_rotation = gmap.get_xyz.detach(), gmap.get_rotation.detach()
            self.get_scaling, self.get_opacity = gmap.get_scaling.detach(), gmap.get_opacity.detach()
            self.get_features = gmap.get_features.detach()
