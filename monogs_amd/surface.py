"""Surface depth: the median depth and the depth variance of a render, the normals of a depth image, and the geometry figures
built on them (``mgs_surface_depth`` / ``mgs_depth_normals``, csrc/surface.hip; DESIGN.md section 3, "Surface depth").

The reference renders one depth, the alpha-blended mean, and never builds a surface from its map.  Here

* ``surface_depth(color)`` walks the lists of the forward that produced ``color`` once more and returns, per pixel, the depth (and
  the index) of the contributor at which the transmittance falls through one half, and the variance of the depth under the blend
  weights -- with an opacity gate and a spread gate on the median;
* ``depth_normals(depth, intr)`` is the camera-frame normal of a metric depth image;
* ``eval_geometry`` sets the mean and the median depth, and the normals of both, against a ground truth over a set of views.

Nothing here is differentiable: the three planes are read-outs.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._launch import _device_guard, _ptr, _stream
from .rasterizer import forward_scratch

WANTS = {"median": _lib.H.MGS_SURFACE_MEDIAN, "variance": _lib.H.MGS_SURFACE_VARIANCE}


class SurfaceDepth(NamedTuple):
    median: Optional[torch.Tensor]        # [H, W] float32; 0: no median, or gated
    median_id: Optional[torch.Tensor]     # [H, W] int32; -1 likewise
    variance: Optional[torch.Tensor]      # [H, W] float32


@torch.no_grad()
def surface_depth(color: torch.Tensor, want: Sequence[str] = ("median", "variance"), min_opacity: float = 0.0,
                  max_std: float = 0.0, want_id: bool = False) -> SurfaceDepth:
    """``median [H, W]``: the view-space depth of the first contributor after which the pixel's transmittance is <= 0.5 (0 where there
    is none); ``median_id`` (with ``want_id``): that Gaussian's index (-1); ``variance``: the variance of the contributors' depths
    under the weights alpha T.  The median and its index are cleared where the forward's opacity is below ``min_opacity`` and, with
    ``max_std > 0`` (which needs ``"variance"``), where the variance exceeds ``max_std ** 2``.

    ``color`` is the colour image of a differentiable ``GaussianRasterizer`` forward: its scratch is found through
    ``color.grad_fn``, as ``render_features`` finds it, so this may be called before or after the rasteriser's own backward (ask once
    before it); that backward is not disturbed."""
    want = tuple(want)
    for w in want:
        if w not in WANTS:
            raise ValueError(f"want must hold names from {tuple(WANTS)}, got {w!r}")
    if not want:
        raise ValueError("want is empty: nothing to compute")
    if want_id and "median" not in want:
        raise ValueError("want_id needs \"median\"")
    if max_std > 0 and "variance" not in want:
        raise ValueError("max_std > 0 gates the median by the variance: add \"variance\" to want")
    t = forward_scratch(color, "surface_depth")
    plane = lambda dt: torch.empty(t.H, t.W, dtype=dt, device=t.device)  # noqa: E731
    median = plane(torch.float32) if "median" in want else None
    median_id = plane(torch.int32) if want_id else None
    variance = plane(torch.float32) if "variance" in want else None
    with _device_guard(t.device):
        _lib.check(_lib.load().mgs_surface_depth(C.byref(t.cam), t.P, t.num_rendered, *t.pointers(), sum(WANTS[w] for w in set(want)),
                                                 float(min_opacity), float(max_std), _ptr(median), _ptr(median_id), _ptr(variance),
                                                 _stream()), "mgs_surface_depth")
    return SurfaceDepth(median, median_id, variance)


@torch.no_grad()
def depth_normals(depth: torch.Tensor, intr, max_jump: float = 0.0) -> torch.Tensor:
    """``[3, H, W]`` float32: the camera-frame normal of the metric depth image ``depth`` ([H, W] or [1, H, W]; <= 0: invalid) by
    central differences of the back-projected pixel centres, facing the camera; zero on the border, next to an invalid pixel and,
    with ``max_jump > 0``, where a neighbour's depth differs from the pixel's by more than that."""
    if not (torch.is_tensor(depth) and depth.is_cuda):
        raise RuntimeError("depth must be a CUDA/HIP tensor; there is no CPU path")
    if depth.dtype != torch.float32:
        raise TypeError(f"depth must be float32 (got {depth.dtype})")
    d = depth.detach().contiguous()
    if d.dim() == 3 and d.shape[0] == 1:
        d = d[0]
    if d.dim() != 2:
        raise ValueError(f"depth must be [H, W] or [1, H, W], got {tuple(depth.shape)}")
    H, W = int(d.shape[0]), int(d.shape[1])
    out = torch.empty(3, H, W, dtype=torch.float32, device=d.device)
    with _device_guard(d.device):
        _lib.check(_lib.load().mgs_depth_normals(W, H, d.data_ptr(), float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy),
                                                 float(max_jump), out.data_ptr(), _stream()), "mgs_depth_normals")
    return out


def render_with_tables(vp, intr, gmap_tensors, bg) -> dict:
    """One ``render()`` of detached map tensors ``(xyz, rot, scales, opac, feat)`` that keeps its tables for ``surface_depth``: the
    colours require a gradient (the forward keeps its scratch for a backward only then) and autograd is on for the call."""
    from .renderer import render
    xyz, rot, scales, opac, feat = gmap_tensors
    with torch.enable_grad():
        return render(vp, intr, xyz, rot, scales, opac, feat.detach().requires_grad_(True), bg)


def _angle_sum(a: torch.Tensor, b: torch.Tensor):
    """(sum of the angles in degrees, count) over the pixels where both unit-normal images [3, H, W] are non-zero."""
    both = (a != 0).any(0) & (b != 0).any(0)
    ang = torch.rad2deg(torch.acos((a * b).sum(0).clamp(-1.0, 1.0))).double()
    return torch.where(both, ang, torch.zeros_like(ang)).sum(), both.sum().double()


@torch.no_grad()
def eval_geometry(gmap, viewpoints, intr, bg, gt_mesh=None, min_opacity: float = 0.9, max_jump: float = 0.05) -> dict:
    """The map's surface against a ground truth, over ``viewpoints``: per view one forward that keeps its tables, ``surface_depth``,
    and ``depth_normals`` of the mean depth (depth / opacity), of the median depth and of the ground truth -- the viewpoint's own
    ``depth``, or ``gt_mesh`` rendered from its pose (``MeshRenderer``).  ``depth_l1_mean_m`` / ``depth_l1_median_m``: mean |d - gt|
    over the pixels with ground truth > 0 and opacity >= ``min_opacity`` (the median's: those that also have a median);
    ``normal_deg_mean`` / ``normal_deg_median``: mean angle to the ground truth's normal over the pixels where both normals are
    non-zero; ``pixels``: the four counts.  The sums stay on the device: ``readbacks`` is 1."""
    from .gaussian_optim import activate
    viewpoints = list(viewpoints)
    dev = gmap._xyz.device
    acc = torch.zeros(8, dtype=torch.float64, device=dev)
    if len(gmap) and viewpoints:
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
        tensors = (gmap._xyz.detach(), rot, scales3, opac, gmap._rgb.detach())
        mr = None
        if gt_mesh is not None:
            from .mesh_render import MeshRenderer
            mr = MeshRenderer(intr, dev)
        for vp in viewpoints:
            pkg = render_with_tables(vp, intr, tensors, bg)
            sd = surface_depth(pkg["render"], want=("median",), min_opacity=min_opacity)
            opacity = pkg["opacity"].detach()[0]
            gt = (mr.render(gt_mesh, vp)["depth"] if mr is not None else vp.depth).to(torch.float32).reshape(opacity.shape)
            seen = (gt > 0) & (opacity >= min_opacity)
            mean = torch.where(seen, pkg["depth"].detach()[0] / opacity.clamp_min(1e-12), torch.zeros_like(opacity))
            has_median = seen & (sd.median > 0)
            zero = torch.zeros_like(opacity)
            n_gt = depth_normals(gt, intr, max_jump)
            a_mean, c_mean = _angle_sum(depth_normals(mean, intr, max_jump), n_gt)
            a_med, c_med = _angle_sum(depth_normals(sd.median, intr, max_jump), n_gt)
            acc += torch.stack([torch.where(seen, (mean - gt).abs(), zero).double().sum(), seen.sum().double(),
                                torch.where(has_median, (sd.median - gt).abs(), zero).double().sum(), has_median.sum().double(),
                                a_mean, c_mean, a_med, c_med])
        if mr is not None:
            acc = torch.cat([acc, mr.status_word().to(torch.float64)])
    row = acc.cpu().tolist()                                            # the ONE read-back
    if len(row) > 8 and int(row[8]) & 1:
        raise Exception("mgs_mesh_render: the ground truth: a triangle names a vertex outside [0, V)")
    ratio = lambda s, c: s / c if c else float("nan")  # noqa: E731
    return dict(depth_l1_mean_m=ratio(row[0], row[1]), depth_l1_median_m=ratio(row[2], row[3]),
                normal_deg_mean=ratio(row[4], row[5]), normal_deg_median=ratio(row[6], row[7]),
                pixels=dict(depth_mean=int(row[1]), depth_median=int(row[3]), normal_mean=int(row[5]), normal_median=int(row[7])),
                views=len(viewpoints), min_opacity=float(min_opacity), max_jump=float(max_jump), readbacks=1)
