"""``MapStep`` -- one optimisation step of the Gaussian map as the window mapper (monogs_amd/mapping.py) and the refiner
(monogs_amd/refinement.py) both take it -- and ``render_map``, the autograd flavour of the same activations for what only renders.

The activations (normalize / exp / sigmoid) are ONE explicit launch into static buffers; the renders differentiate with respect
to five detached leaves (xyz, rgb, activated opacity, scales, rotation: the order in which the rasteriser's backward lays their
gradients out back to back); ``apply`` takes the five gradients from wherever the driver gathered them and steps the map.  Nothing
here synchronises the host, allocates outside the caching allocator or launches a memset / memcpy node: all of it may be captured.
"""
from __future__ import annotations

import torch

from . import _lib
from .gaussian_map import GaussianMap
from .gaussian_optim import activate, activate_backward_into, activate_into
from ._launch import _device_guard, _stream
from .rasterizer import GaussianRasterizer
from .renderer import raster_settings, render


def render_map(vp, intr, gmap: GaussianMap, bg):
    """``render()`` with the map's activations (normalize / exp / sigmoid, forward and backward) in one launch each."""
    if gmap.fused_adam and gmap._rotation.requires_grad:
        rot, scales3, opac = activate(gmap._rotation, gmap._scaling, gmap._opacity)
        return render(vp, intr, gmap.get_xyz, rot, scales3, opac, gmap.get_features, bg)
    return render(vp, intr, gmap.get_xyz, gmap.get_rotation, gmap.get_scaling, gmap.get_opacity, gmap.get_features, bg)


def rasterize(intr, bg, cam3, leaves, holder, theta, rho):
    """The rasteriser call of ``render()`` (/root/reference/gaussian_splatting/gaussian_renderer/__init__.py:52-156) on five tensors
    in the order of ``MapStep.leaves``; ``holder``: the caller's zeros whose ``.grad`` receives dL/dmean2D; ``cam3``: the camera."""
    xyz, feat, opac, scales3, rot = leaves
    color, radii, depth, _, n_touched = GaussianRasterizer(raster_settings(intr, bg, *cam3))(
        means3D=xyz, means2D=holder, opacities=opac, colors_precomp=feat, scales=scales3, rotations=rot, theta=theta, rho=rho,
        intr=getattr(intr, "delta", None))
    return color, radii, depth, n_touched


class MapStep:
    """Buffers for one map size (a driver drops its ``MapStep`` when ``len(gmap)`` changes) and the launches around the renders."""

    def __init__(self, gmap: GaussianMap):
        self.gmap = gmap
        P, f32 = len(gmap), dict(dtype=torch.float32, device=gmap.device)
        self.P, self.sd = P, int(gmap._scaling.shape[1])
        self.rot, self.scales3, self.opac = torch.empty(P, 4, **f32), torch.empty(P, 3, **f32), torch.empty(P, 1, **f32)
        self.d_rot, self.d_scale, self.d_opac = torch.empty(P, 4, **f32), torch.empty(P, self.sd, **f32), torch.empty(P, 1, **f32)
        self.iter_dev = torch.zeros(1, dtype=torch.int32, device=gmap.device)      # the iteration count the schedule steps

    def activate(self):
        gmap = self.gmap
        activate_into(gmap._rotation, gmap._scaling, gmap._opacity, self.rot, self.scales3, self.opac)

    def leaves(self):
        """The five tensors the renders differentiate with respect to: leaves that CUT the graph at the activations (their
        backward is one explicit launch in ``apply``)."""
        gmap = self.gmap
        return [t.detach().requires_grad_(True) for t in (gmap._xyz, gmap._rgb, self.opac, self.scales3, self.rot)]

    def set_iteration(self, n: int):
        """Device copies of the driver's iteration count and of the learning rates (what the schedule in ``apply`` steps)."""
        self.iter_dev.fill_(n)
        self.gmap.optimizer.device_lrs()

    def apply(self, grads, before_step=None, schedule: bool = True):
        """``grads``: the gradients of the five ``leaves()``, in their order.  ``before_step`` runs between the assignment of the
        raw parameters' ``.grad`` and the Adam step (map surgery, clones for tests); what it returns is returned."""
        g_xyz, g_rgb, g_opac, g_scales3, g_rot = grads
        gmap, lib = self.gmap, _lib.load()
        activate_backward_into(gmap._rotation, self.scales3, self.opac, g_rot, g_scales3, g_opac, self.sd,
                               self.d_rot, self.d_scale, self.d_opac)
        # the leaves' gradients, exactly where autograd would have put them -- BEFORE any surgery: densify_and_prune replaces
        # every tensor (new leaves, no gradient: no step, as torch.optim.Adam), an opacity reset replaces the opacities only
        for q, g in zip(gmap.params(), (g_xyz, g_rgb, self.d_opac, self.d_scale, self.d_rot)):
            q.grad = g
        out = before_step() if before_step is not None else None
        gmap.optimizer.step()                     # (after surgery every .grad is None: no step, as torch.optim.Adam)
        s = gmap.lr_schedule
        if schedule and s is not None:            # update_learning_rate(iteration), AFTER the step, on the device
            with _device_guard(gmap._xyz.device):
                _lib.check(lib.mgs_lr_schedule_step(
                    self.iter_dev.data_ptr(), gmap.optimizer.device_lrs().data_ptr(), float(s["lr_init"]), float(s["lr_final"]),
                    int(s.get("lr_delay_steps", 0)), float(s.get("lr_delay_mult", 1.0)), int(s["max_steps"]), _stream()),
                    "mgs_lr_schedule_step")
        return out
