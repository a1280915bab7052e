"""Monocular operation: frames without measured depth, and the depth hypothesis a new keyframe is back-projected from.

A [RECALL] of public upstream MonoGS (``add_new_keyframe``, ``get_loss_tracking_rgb``, ``get_loss_mapping_rgb``): the reference
fork removed that code in its rewrite and keeps only what it used -- ``get_median_depth(..., return_std=True)``
(/root/reference/utils/slam_utils.py:149-157), ``rgb_boundary_threshold: 0.01`` in every config and the commented-out
``self.monocular`` switches (utils/slam_mapper.py:47-53,166,442; utils/slam_tracker.py:77).  Parity is therefore unpinned; the
specification is written down in DESIGN.md ("Monocular operation") and checked against a float64 restatement
(tests/monocular_mirror.py).  The two RGB-only losses live in ``fused_losses``; here:

* ``valid_rgb``: the pixels that carry colour (``rgb.sum(0) > rgb_boundary_threshold``) -- what upstream masks its RGB losses
  and its depth hypothesis with;
* ``pseudo_depth``: one stream-ordered call (``mgs_pseudo_depth``, csrc/monodepth.hip; no host read-back, capturable) from a
  keyframe's frozen render to the image ``create_viewpoint_pcd(depth=...)`` back-projects -- the rendered depth where it lies
  within one standard deviation of the median, the median elsewhere, both with noise in proportion to the deviation; without a
  render (the first frame) or with fewer than two valid pixels ``init_mean + init_sigma * noise``;
* ``monocular_frames``: depthless copies of RGB-D frames.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from .frames import Viewpoint
from ._launch import _device_guard, _stream

PSEUDO_DEPTH_DEFAULTS = dict(init_mean=2.0, init_sigma=0.3, opacity_min=0.95, sigma_in=0.2, sigma_out=0.5)


def valid_rgb(rgb: torch.Tensor, rgb_boundary_threshold: float = 0.01) -> torch.Tensor:
    """bool[H,W]: ``rgb.sum(0) > rgb_boundary_threshold`` (the black border an undistorted image brings carries no colour)."""
    return rgb.sum(dim=0) > rgb_boundary_threshold


def is_monocular(viewpoint) -> bool:
    return getattr(viewpoint, "sensor", "depth") == "monocular"


def window_is_monocular(viewpoints: Sequence) -> bool:
    """The sensor of a mapping window; a window that mixes sensors is an error (its keyframes would be optimised by different losses)."""
    kinds = {is_monocular(v) for v in viewpoints}
    if len(kinds) > 1:
        raise ValueError("the window mixes monocular and depth keyframes")
    return bool(kinds) and kinds.pop()


def _image(t: torch.Tensor, shape, what: str) -> torch.Tensor:
    if t.device.type != "cuda":
        raise RuntimeError(f"pseudo_depth: no CPU path ({what} must be a device tensor)")
    t = t.detach()
    if t.numel() != shape[0] * shape[1]:
        raise ValueError(f"pseudo_depth: {what} has {t.numel()} elements, the image {shape[0]} x {shape[1]}")
    return t.to(torch.float32).contiguous()


@torch.no_grad()
def pseudo_depth(render_depth: Optional[torch.Tensor], render_opacity: Optional[torch.Tensor], valid_rgb: Optional[torch.Tensor],
                 generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None, shape=None, **params):
    """``(depth [H,W], stats [4])``, both on the device: the depth hypothesis of ``mgs_pseudo_depth`` (include/monogs_raster.h) and
    ``(median, std, count, used_init_rule)``.  ``render_depth=None``: the init rule.  ``noise``: [H,W] standard normals; default
    ``torch.randn`` from ``generator`` (a DEVICE generator; under graph capture bring ``noise``).  ``shape``: ``(H, W)`` when neither
    a render, a ``valid_rgb`` nor ``noise`` gives it.  ``params``: ``PSEUDO_DEPTH_DEFAULTS``."""
    unknown = set(params) - set(PSEUDO_DEPTH_DEFAULTS)
    if unknown:
        raise TypeError(f"pseudo_depth: unknown parameter(s) {sorted(unknown)}")
    lib = _lib.load()
    ref = next((t for t in (render_depth, valid_rgb, noise) if t is not None), None)
    if ref is None and shape is None:
        raise ValueError("pseudo_depth: nothing gives the image size (render_depth, valid_rgb, noise or shape)")
    H, W = (int(x) for x in (ref.shape[-2:] if ref is not None else shape))
    dev = ref.device if ref is not None else (generator.device if generator is not None else torch.device("cuda"))
    if noise is None:
        noise = torch.randn(H, W, device=dev, generator=generator)
    z = _image(noise, (H, W), "noise")
    d = None if render_depth is None else _image(render_depth, (H, W), "render_depth")
    o = None if render_opacity is None or d is None else _image(render_opacity, (H, W), "render_opacity")
    ok = None
    if valid_rgb is not None:
        if valid_rgb.numel() != H * W:
            raise ValueError("pseudo_depth: valid_rgb does not have the image's size")
        ok = valid_rgb.contiguous().view(torch.uint8) if valid_rgb.dtype == torch.bool else (valid_rgb != 0).to(torch.uint8).contiguous()
    prm = _lib.MgsPseudoDepthParams(**{k: float(v) for k, v in dict(PSEUDO_DEPTH_DEFAULTS, **params).items()})
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with _device_guard(z.device):
        out = torch.empty(H, W, dtype=torch.float32, device=z.device)
        stats = torch.empty(4, dtype=torch.float32, device=z.device)
        scratch = None if d is None else torch.empty(lib.mgs_pseudo_depth_scratch_bytes(H * W), dtype=torch.uint8, device=z.device)
        _lib.check(lib.mgs_pseudo_depth(W, H, p(d), p(o), p(ok), p(z), C.byref(prm), p(scratch), p(out), p(stats), _stream()),
                   "mgs_pseudo_depth")
    return out, stats


def monocular_frames(frames: Sequence, rgb_boundary_threshold: float = 0.01):
    """Depthless copies of RGB-D frames: the colour image, the ground-truth pose, ``mask`` (and-ed with ``valid_rgb``), ``grad_mask``
    and segmentation are kept (shared, not copied), the current pose is carried over, the depth is ONE all-zero image shared by
    all of them."""
    if not frames:
        return []
    zero = torch.zeros_like(frames[0].depth, dtype=torch.float32)
    out = []
    for f in frames:
        vp = Viewpoint(f.frame_idx, f.rgb, zero if zero.shape == f.depth.shape else None, f.device, gt_R=f.R_gt, gt_T=f.T_gt,
                       mask=f.mask, grad_mask=f.grad_mask, segmentation=getattr(f, "segmentation", None), sensor="monocular",
                       rgb_boundary_threshold=rgb_boundary_threshold)
        vp.update_RT(f.R.clone(), f.T.clone())
        out.append(vp)
    return out
