"""K-channel feature rendering: per-Gaussian rows (object probabilities, semantic logits, ...) blended per pixel through the
lists and decisions a rasteriser forward already built (``mgs_features_forward`` / ``mgs_features_backward``,
csrc/features.hip).

The reference keeps a row of object probabilities per Gaussian (gaussian_splatting/scene/gaussian_model.py:47-66) and only ever
shows its per-Gaussian argmax (viewer/viewer_packet.py:52-54); it leaves "set requires grad to True" as a TODO (:381).  Here

* ``render_features(color, features)`` blends ``features [P, K]`` with the weights alpha T of the forward that produced
  ``color`` -- no preprocess, no sort, no second blend decision -- and is differentiable in ``features``;
* ``FeatureRasterizer`` is the stand-alone form for a caller without a colour render (a viewer, an evaluation).

There is no gradient to the background, the geometry, the opacities or the pose: the feature image is a read-out of a map that
the colour and depth losses shape.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._launch import _device_guard, _ptr, _stream
from .rasterizer import ForwardScratch, GaussianRasterizationSettings, GaussianRasterizer, forward_scratch

MAX_FEATURE_CHANNELS = _lib.H.MGS_MAX_FEATURE_CHANNELS


def _check(t: ForwardScratch, features, bg) -> int:
    """Shape, dtype and device errors, raised before the library is touched.  Returns K."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2:
        raise ValueError("features must be a [P, K] tensor")
    if features.shape[0] != t.P:
        raise ValueError(f"features has {features.shape[0]} rows, the forward rendered {t.P} Gaussians")
    K = int(features.shape[1])
    if not 1 <= K <= MAX_FEATURE_CHANNELS:
        raise ValueError(f"K = {K}: features must have 1..{MAX_FEATURE_CHANNELS} channels")
    for name, x in (("features", features), ("bg", bg)):
        if x is None:
            continue
        if x.dtype != torch.float32:
            raise TypeError(f"{name} must be float32 (got {x.dtype})")
        if x.device != t.device:
            raise RuntimeError(f"{name} is on {x.device}, the forward ran on {t.device}")
    if bg is not None and (bg.dim() != 1 or bg.shape[0] != K):
        raise ValueError(f"bg must have K = {K} entries (got shape {tuple(bg.shape)})")
    return K


class _RenderFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, t: ForwardScratch, bg, want_labels, min_opacity):
        lib = _lib.load()
        f = features.detach().contiguous()
        K = int(f.shape[1])
        bg_ = None if bg is None else bg.detach().contiguous()
        out = torch.empty(K, t.H, t.W, dtype=torch.float32, device=t.device)
        labels = torch.empty(t.H, t.W, dtype=torch.int32, device=t.device) if want_labels else None
        with _device_guard(t.device):
            _lib.check(lib.mgs_features_forward(C.byref(t.cam), t.P, K, t.num_rendered, *t.pointers(), f.data_ptr(),
                                                _ptr(bg_), out.data_ptr(), _ptr(labels), float(min_opacity), _stream()),
                       "mgs_features_forward")
        ctx.tables, ctx.K = t, K
        if labels is None:
            return out
        ctx.mark_non_differentiable(labels)
        return out, labels

    @staticmethod
    def backward(ctx, grad_out, grad_labels=None):
        return features_backward(ctx.tables, grad_out, ctx.K), None, None, None, None


def features_backward(t: ForwardScratch, d_out: torch.Tensor, K: int) -> torch.Tensor:
    """``mgs_features_backward`` on the handle ``t`` (``forward_scratch(color)``): ``d_features [P, K]`` from ``d_out [K, H, W]``.  What the
    autograd node's backward runs; a loop that steps the rows itself (``object_layer.ObjectLayerTrainer``) calls it directly."""
    lib = _lib.load()
    g = d_out.to(torch.float32).contiguous()
    d_feat = torch.empty(t.P, K, dtype=torch.float32, device=t.device)
    with _device_guard(t.device):
        _lib.check(lib.mgs_features_backward(C.byref(t.cam), t.P, K, t.num_rendered, *t.pointers(), g.data_ptr(),
                                             d_feat.data_ptr(), _stream()), "mgs_features_backward")
    return d_feat


def render_features(color: torch.Tensor, features: torch.Tensor, bg: Optional[torch.Tensor] = None,
                    want_labels: bool = False, min_opacity: float = 0.5):
    """``feat[K, H, W] = sum_i features[g_i] alpha_i T_i (+ final_T bg)`` over the contributors the forward behind ``color``
    blended; with ``want_labels`` also ``labels[H, W]`` (int32): the lowest-index argmax over the K channels without the
    background term, -1 where that forward's opacity is below ``min_opacity``.

    ``color`` is the colour image of a differentiable ``GaussianRasterizer`` forward: its scratch is found through
    ``color.grad_fn`` and referenced from here on, so this may be called again, and ``features.grad`` obtained, after the
    rasteriser's own backward has run; that backward is not disturbed.  Differentiable in ``features`` only."""
    t = forward_scratch(color, "render_features")
    _check(t, features, bg)
    return _RenderFeatures.apply(features, t, bg, bool(want_labels), float(min_opacity))


class FeatureRasterizer(torch.nn.Module):
    """Stand-alone feature render: one forward of its own (geometry detached, a dummy colour), then ``render_features``.
    Returns a dict with ``features [K,H,W]``, ``depth``, ``opacity``, ``radii``, ``n_touched`` (and ``labels``)."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, opacities, features, scales=None, rotations=None, cov3D_precomp=None, bg=None,
                want_labels=False, min_opacity=0.5):
        d = lambda x: None if x is None else x.detach()  # noqa: E731
        means3D = means3D.detach()
        # (requires_grad: the forward keeps its tables for a backward only then -- they are what render_features reads)
        dummy = torch.zeros(means3D.shape[0], 3, dtype=torch.float32, device=means3D.device, requires_grad=True)
        color, radii, depth, opacity, n_touched = GaussianRasterizer(self.raster_settings)(
            means3D=means3D, means2D=torch.zeros_like(means3D), opacities=d(opacities), colors_precomp=dummy,
            scales=d(scales), rotations=d(rotations), cov3D_precomp=d(cov3D_precomp))
        res = render_features(color, features, bg=bg, want_labels=want_labels, min_opacity=min_opacity)
        out = dict(depth=depth.detach(), opacity=opacity.detach(), radii=radii, n_touched=n_touched)
        if want_labels:
            out["features"], out["labels"] = res
        else:
            out["features"] = res
        return out
