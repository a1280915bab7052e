"""Pose-tangent rendering and the normal equations of the tracking loss (``mgs_pose_jacobian`` / ``mgs_gn_normal_equations``,
csrc/pose_tangent.hip and csrc/gauss_newton.hip).

The reference's tracker (/root/reference/utils/slam_tracker.py:142-176) only ever sees the summed gradient of its loss; a
Gauss-Newton step needs the per-pixel Jacobian of the render with respect to the six pose tangents, a forward-mode pass:

* ``pose_jacobian(color)`` walks the lists of the forward that produced ``color`` once more and returns ``J [6, 5, H, W]``:
  ``J[k, c] = d (R, G, B, depth, opacity)[c] / d tau_k``, ``tau = (rho, theta)`` of ``T_cw(tau) = exp(tau^) T_cw`` at 0;
* ``normal_equations(J, color, depth, opacity, viewpoint, ...)`` forms ``H [8, 8]``, ``g [8]``, the robust cost and the two row
  counts of ``get_loss_tracking``'s rows in the unknowns ``(rho, theta, exposure_a, exposure_b)`` on the device, in double.

``pose_optim.PoseGaussNewton`` solves and retracts; ``gn_tracking`` is the tracker built on the three.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .fused_losses import _RGB_ONLY, _TRACKING, _u8
from ._launch import _device_guard, _f32, _stream
from .rasterizer import forward_scratch

SYSTEM_DOUBLES = _lib.H.MGS_GN_SYSTEM_DOUBLES          # H[8][8], g[8], E, N_rgb, N_d


@torch.no_grad()
def pose_jacobian(color: torch.Tensor) -> torch.Tensor:
    """``J [6, 5, H, W]`` (float32) of the forward behind ``color``, the colour image of a differentiable ``GaussianRasterizer``
    forward that took ``colors_precomp``.  The forward's scratch and inputs are found through ``color.grad_fn``; they are only read,
    so the rasteriser's own backward may follow (or, after one ``forward_scratch(color)`` request, come first) undisturbed.
    Decisions are constants, a clamped view-space ratio is a constant and the 0.99 cap of alpha is straight-through, as in the
    backward: ``sum_p <g[:4, p], J[k, :4, p]>`` is the backward's ``dL/dtau_k`` for any cotangent images ``g``."""
    who = "pose_jacobian"
    t = forward_scratch(color, who)
    fn = color.grad_fn
    try:
        means3D, _, _, _, sc_, rot_, cov_, radii, _, _ = fn.saved_tensors
    except RuntimeError as e:
        raise RuntimeError(f"{who}: the rasteriser's backward has already freed this forward's scratch; "
                           f"call {who} once before that backward to keep it") from e
    has_sh, _, has_sr, has_cov, _, _ = fn.has
    if has_sh:
        raise RuntimeError(f"{who}: the forward used SH colours, which depend on the camera position; only colors_precomp is supported")
    lib = _lib.load()
    J = torch.empty(6, 5, t.H, t.W, dtype=torch.float32, device=t.device)
    with _device_guard(t.device):
        scratch = torch.empty(lib.mgs_pose_tangent_bytes(t.P), dtype=torch.uint8, device=t.device)
        _lib.check(lib.mgs_pose_jacobian(C.byref(t.cam), t.P, t.num_rendered, means3D.data_ptr(),
                                         sc_.data_ptr() if has_sr else None, rot_.data_ptr() if has_sr else None,
                                         cov_.data_ptr() if has_cov else None, radii.data_ptr(), *t.pointers(),
                                         scratch.data_ptr(), J.data_ptr(), _stream()), "mgs_pose_jacobian")
    return J


class NormalEquations:
    """The device system of ``normal_equations``: ``buf`` holds 75 doubles; the properties are views."""
    __slots__ = ("buf",)

    def __init__(self, buf):
        self.buf = buf

    @property
    def H(self) -> torch.Tensor:
        return self.buf[:64].view(8, 8)

    @property
    def g(self) -> torch.Tensor:
        return self.buf[64:72]

    @property
    def cost(self) -> torch.Tensor:
        return self.buf[72]

    @property
    def n_rgb(self) -> torch.Tensor:
        return self.buf[73]

    @property
    def n_depth(self) -> torch.Tensor:
        return self.buf[74]


@torch.no_grad()
def normal_equations(J, color, depth, opacity, viewpoint, delta_rgb: float = 0.05, delta_depth: float = 0.05,
                     rgb_only: bool = False, out: NormalEquations = None) -> NormalEquations:
    """``H = sum s omega j j^T``, ``g = sum s omega r j`` and the Huber cost over the rows of ``get_loss_tracking``
    (/root/reference/utils/slam_utils.py:58-98) -- colour rows ``e^a C + b - I`` on ``mask grad_mask (opacity > 0.99)`` with
    ``s = 0.5 / 3HW``, depth rows ``D - D_gt`` on ``(D_gt > 0) (opacity > 0.99)`` with ``s = 1 / N_d`` -- in the unknowns
    ``(rho, theta, a, b)``; the reference's factor ``mean(opacity)`` is dropped.  ``omega`` is the Huber weight of the residual
    at ``delta_rgb`` / ``delta_depth``.  ``rgb_only``: no depth rows (monocular viewpoints).  Two launches, no host
    synchronisation, bitwise reproducible.  ``out``: a system to overwrite (a captured loop keeps one)."""
    lib = _lib.load()
    render = _f32(color.detach(), "color")
    H, W = int(render.shape[-2]), int(render.shape[-1])
    dev = render.device
    Jc = _f32(J, "J")
    if Jc.numel() != 30 * H * W:
        raise ValueError(f"J must hold 30 planes of {H} x {W} (got shape {tuple(J.shape)})")
    dep = None if rgb_only else _f32(depth.detach(), "depth")
    opac = _f32(opacity.detach(), "opacity")
    gt_rgb = _f32(viewpoint.rgb, "viewpoint.rgb")
    gt_depth = None if rgb_only else _f32(viewpoint.depth, "viewpoint.depth")
    a, b = _f32(viewpoint.exposure_a.detach(), "exposure_a"), _f32(viewpoint.exposure_b.detach(), "exposure_b")
    mask, gm = _u8(viewpoint.mask), _u8(viewpoint.grad_mask)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with _device_guard(dev):
        if out is None:
            out = NormalEquations(torch.empty(SYSTEM_DOUBLES, dtype=torch.float64, device=dev))
        scratch = torch.empty(lib.mgs_gn_scratch_bytes(W, H) // 8, dtype=torch.float64, device=dev)
        _lib.check(lib.mgs_gn_normal_equations(W, H, _TRACKING | (_RGB_ONLY if rgb_only else 0), p(Jc), p(render), p(dep), p(opac),
                                               p(gt_rgb), p(gt_depth), p(mask), p(gm), p(a), p(b), float(delta_rgb),
                                               float(delta_depth), p(scratch), p(out.buf), _stream()),
                   "mgs_gn_normal_equations")
    return out
