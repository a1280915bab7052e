"""Learning and scoring the map's object layer: the fused label loss (``mgs_label_loss_grads``), a trainer that fuses a
keyframe's segmentation into the per-Gaussian rows over every view that sees them, and label accuracy / IoU from a confusion
matrix counted on the device (``mgs_label_confusion``); csrc/labels.hip.

The reference leaves the rows as the one-hot id of the pixel a Gaussian was back-projected from ("set requires grad to True" is
a TODO at gaussian_splatting/scene/gaussian_model.py:381) and measures no label accuracy.  Here the RAW rows ``_obj_prob`` are
logits: ``render_features`` blends them per pixel, the loss is the softmax cross-entropy of that image against the keyframe's
8-bit ids, ``mgs_features_backward`` carries its gradient to the rows and ``GaussianMap.object_optimizer`` (Adam) steps them.
Nothing else of the map takes a gradient from the labels: geometry, opacity and colour are detached in the forward.

* ``LabelTarget`` / ``label_loss_grads`` / ``get_loss_labels``: the loss, hand-driven or as an autograd scalar;
* ``label_confusion`` / ``segmentation_scores`` / ``eval_segmentation``: the score;
* ``ObjectLayerTrainer``: one forward, one feature render, the loss, the feature backward and one Adam step per call.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._launch import _device_guard, _f32, _ptr, _stream

MAX_OBJECTS = _lib.H.MGS_MAX_FEATURE_CHANNELS           # ids are 8-bit
_LOSS = _lib.H.MGS_LABEL_SCRATCH_LOSS                   # a float index


def _no_cpu(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: no CPU path (the label kernels are HIP only)")


def _check_k(K) -> int:
    K = int(K)
    if not 1 <= K <= MAX_OBJECTS:
        raise ValueError(f"K = {K}: the label kernels take 1..{MAX_OBJECTS} channels")
    return K


def _scratch(dev) -> torch.Tensor:
    return torch.empty(_lib.load().mgs_label_scratch_bytes() // 4, dtype=torch.float32, device=dev)


class LabelTarget:
    """The constants of a keyframe's label loss: ``labels`` as a contiguous uint8 ``[H, W]`` image, ``valid`` (uint8, or None =
    every pixel) and, per K, the device count ``{N, H W - N}`` of the pixels that count (``valid`` non-zero and id < K;
    ``mgs_label_prepare``, once per K).  ``labels``: an int / long / uint8 ``[H, W]`` device tensor; an id outside 0..255 raises
    ``ValueError`` (that check reads an int tensor back once, here and never per iteration)."""

    def __init__(self, labels: torch.Tensor, valid: Optional[torch.Tensor] = None):
        if not torch.is_tensor(labels) or labels.dim() != 2:
            raise ValueError("labels must be an [H, W] tensor")
        if labels.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise TypeError(f"labels must be an integer tensor (got {labels.dtype})")
        if labels.dtype != torch.uint8 and labels.numel():
            lo, hi = (int(v) for v in torch.stack((labels.min(), labels.max())).tolist())
            if lo < 0 or hi > 255:
                raise ValueError(f"label ids must lie in 0..255 (got {lo}..{hi}): ids are 8-bit, mask other pixels with `valid`")
        _no_cpu(labels, "LabelTarget")
        if valid is not None:
            _no_cpu(valid, "LabelTarget")
            if tuple(valid.shape) != tuple(labels.shape) or valid.device != labels.device:
                raise ValueError(f"valid must be an [H, W] image like labels (got {tuple(valid.shape)} on {valid.device})")
            valid = valid.contiguous().view(torch.uint8) if valid.dtype == torch.bool else (valid != 0).to(torch.uint8).contiguous()
        self.labels = labels.detach().to(torch.uint8).contiguous()
        self.valid = valid
        self.H, self.W = int(labels.shape[0]), int(labels.shape[1])
        self.device = labels.device
        self._counts: Dict[int, torch.Tensor] = {}

    def count(self, K: int) -> torch.Tensor:
        """Device uint32 view ``{N, H W - N}`` (an int32 tensor of two elements) for a loss over K channels."""
        K = _check_k(K)
        c = self._counts.get(K)
        if c is None:
            lib = _lib.load()
            c = torch.empty(2, dtype=torch.int32, device=self.device)
            with _device_guard(self.device):
                _lib.check(lib.mgs_label_prepare(self.W, self.H, K, self.labels.data_ptr(), _ptr(self.valid),
                                                 _scratch(self.device).data_ptr(), c.data_ptr(), _stream()), "mgs_label_prepare")
            self._counts[K] = c
        return c


class LabelGrads:
    """Result of ``label_loss_grads``: ``d_feat [K, H, W]`` and views of the device scalars ``loss`` and ``count`` (N)."""
    __slots__ = ("d_feat", "scratch", "_count")

    def __init__(self, d_feat, scratch, count):
        self.d_feat, self.scratch, self._count = d_feat, scratch, count

    @property
    def loss(self) -> torch.Tensor:
        return self.scratch[_LOSS]

    @property
    def count(self) -> torch.Tensor:
        return self._count[0]


def _check_feat(feat, target: LabelTarget) -> int:
    _no_cpu(feat, "label_loss_grads")
    if not isinstance(target, LabelTarget):
        raise TypeError("target must be a LabelTarget")
    if feat.dim() != 3:
        raise ValueError("feat must be a [K, H, W] tensor")
    K = _check_k(feat.shape[0])
    if tuple(feat.shape[1:]) != (target.H, target.W) or feat.device != target.device:
        raise ValueError(f"feat is {tuple(feat.shape)} on {feat.device}, the target {target.H} x {target.W} on {target.device}")
    return K


@torch.no_grad()
def label_loss_grads(feat: torch.Tensor, target: LabelTarget) -> LabelGrads:
    """Softmax cross-entropy of ``feat [K, H, W]`` (logits: ``render_features`` of the raw rows, no background) against
    ``target``, VALUE + GRADIENT in two launches and no host synchronisation, as ``fused_losses.loss_grads`` is for the SLAM
    losses: ``L = mean over the counted pixels of logsumexp_k feat - feat[label]``, ``d_feat = (softmax - onehot) / N`` there
    and exactly 0 elsewhere; no counted pixel: L = 0, d_feat = 0."""
    K = _check_feat(feat, target)
    lib = _lib.load()
    f = _f32(feat.detach(), "feat")        # (a dense view that starts inside a buffer stays: the kernels choose their route by the address)
    with _device_guard(f.device):
        count = target.count(K)
        scratch = _scratch(f.device)
        d_feat = torch.empty(K, target.H, target.W, dtype=torch.float32, device=f.device)
        _lib.check(lib.mgs_label_loss_grads(target.W, target.H, K, f.data_ptr(), target.labels.data_ptr(), _ptr(target.valid),
                                            count.data_ptr(), scratch.data_ptr(), d_feat.data_ptr(), _stream()),
                   "mgs_label_loss_grads")
    return LabelGrads(d_feat, scratch, count)


class _LabelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, target):
        g = label_loss_grads(feat, target)
        ctx.save_for_backward(g.d_feat)
        return g.loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (d_feat,) = ctx.saved_tensors
        return d_feat * grad_out, None


def get_loss_labels(feat: torch.Tensor, target: LabelTarget) -> torch.Tensor:
    """The label loss as an autograd scalar, as ``get_loss_mapping`` is for the mapping loss: the forward runs the fused value +
    gradient call and keeps the gradient image, ``backward`` scales it by the incoming gradient."""
    _check_feat(feat, target)
    return _LabelLoss.apply(feat, target)


@torch.no_grad()
def label_confusion(pred: torch.Tensor, target: LabelTarget, K: int, out=None):
    """ADDS one frame into ``(counts [K, K], side [2])`` (int32 tensors holding uint32 counts; made and zeroed when ``out`` is
    None) and returns the pair: ``counts[gt, pred]`` over the counted pixels with a prediction, ``side = {counted pixels whose
    ``pred`` is -1 (not seen), pixels not counted}``.  ``pred``: int32 ``[H, W]``, the ``labels`` of ``render_features``."""
    if not isinstance(target, LabelTarget):
        raise TypeError("target must be a LabelTarget")
    K = _check_k(K)
    _no_cpu(pred, "label_confusion")
    if pred.dtype != torch.int32 or tuple(pred.shape) != (target.H, target.W) or pred.device != target.device:
        raise ValueError(f"pred must be int32 [{target.H}, {target.W}] on {target.device} (got {pred.dtype} {tuple(pred.shape)})")
    dev = pred.device
    if out is None:
        out = (torch.zeros(K, K, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
    counts, side = out
    for t, shape, what in ((counts, (K, K), "counts"), (side, (2,), "side")):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out: {what} must be a contiguous int32 {shape} tensor on {dev}")
    lib = _lib.load()
    with _device_guard(dev):
        _lib.check(lib.mgs_label_confusion(target.W, target.H, K, pred.contiguous().data_ptr(), target.labels.data_ptr(),
                                           _ptr(target.valid), counts.data_ptr(), side.data_ptr(), _stream()), "mgs_label_confusion")
    return out


def segmentation_scores(counts) -> Dict:
    """``pixel_accuracy`` (trace / sum), ``iou`` (per class: TP / (TP + FP + FN), NaN for a class that occurs neither in the
    ground truth nor in the prediction), ``miou`` (mean over the classes that occur) and ``classes`` (how many do) from a
    confusion matrix ``[gt, pred]`` (tensor or array; uint32 counts read from an int32 tensor are taken as unsigned).  Host
    arithmetic in float64, once, after the read-back."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"a confusion matrix is square (got {c.shape})")
    if c.dtype == np.int32:
        c = c.view(np.uint32)
    c = c.astype(np.float64)
    tp, total = np.diag(c), c.sum()
    union = c.sum(0) + c.sum(1) - tp
    present = union > 0
    iou = np.full(c.shape[0], np.nan)
    iou[present] = tp[present] / union[present]
    return dict(pixel_accuracy=float(tp.sum() / total) if total > 0 else float("nan"),
                miou=float(iou[present].mean()) if present.any() else float("nan"),
                iou=[float(v) for v in iou], classes=int(present.sum()))


# ---- rendering the rows ----------------------------------------------------------------------------------------------------
def _frozen_geometry(gmap):
    from .gaussian_optim import activate
    with torch.no_grad():
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
    return gmap._xyz.detach(), rot, scales3, opac


def _forward_tables(vp, intr, geometry, bg):
    """One rasteriser forward with detached geometry and a dummy colour (what ``FeatureRasterizer`` does) through ``render()``,
    so that the camera tensors are the cached ones; returns the tables the feature kernels read."""
    from .rasterizer import forward_scratch
    from .renderer import render
    xyz, rot, scales3, opac = geometry
    # (requires_grad: the forward keeps its tables for a backward only then)
    dummy = torch.zeros(xyz.shape[0], 3, dtype=torch.float32, device=xyz.device, requires_grad=True)
    pkg = render(vp, intr, xyz, rot, scales3, opac, dummy, bg)
    return forward_scratch(pkg["render"], "render_features"), pkg


def _target_of(vp) -> LabelTarget:
    seg = getattr(vp, "segmentation", None)
    if seg is None:
        raise ValueError(f"frame {getattr(vp, 'frame_idx', '?')} carries no segmentation")
    return LabelTarget(seg)


class ObjectLayerTrainer:
    """Fuses the keyframes' segmentation into the rows of a ``GaussianMap(nr_objects=K, learn_objects=True)``.

    ``step(viewpoint)``: one rasteriser forward with detached geometry, ``render_features`` on the raw rows, the fused label
    loss, ``mgs_features_backward`` and one Adam step on the rows.  The step adds no host synchronisation of its own: the frame's
    ``LabelTarget`` comes from a cache per frame index (``run`` fills it before its loop, a first ``step`` on a new frame builds
    it), the count N and the loss stay on the device, and what is left is the rasteriser forward's own read-back of its instance
    count on the exact path -- none under ``rasterizer.set_sync_free(True)``.  Returns the loss as a device scalar.  ``last_grad``: the row gradient the last step handed to Adam.  No parameter but
    the rows is touched, and the map's own optimiser is not stepped."""

    def __init__(self, gmap, intr, bg):
        if gmap.nr_objects is None or not getattr(gmap, "learn_objects", False):
            raise ValueError("ObjectLayerTrainer needs GaussianMap(nr_objects=K, learn_objects=True)")
        if not torch.device(gmap.device).type == "cuda":
            raise RuntimeError("ObjectLayerTrainer: no CPU path (the label kernels are HIP only)")
        self.gmap, self.intr, self.bg = gmap, intr, bg
        self.targets: Dict[int, LabelTarget] = {}
        self.last_grad = None
        self.steps = 0

    def target(self, vp) -> LabelTarget:
        key = int(vp.frame_idx)
        t = self.targets.get(key)
        if t is None:
            t = self.targets[key] = _target_of(vp)
            t.count(self.gmap.nr_objects)
        return t

    def step(self, vp) -> torch.Tensor:
        from .feature_render import features_backward, render_features
        gmap = self.gmap
        if gmap.object_optimizer is None or len(gmap) == 0:
            raise RuntimeError("the map has no rows to learn yet")
        target = self.target(vp)
        tables, pkg = _forward_tables(vp, self.intr, _frozen_geometry(gmap), self.bg)
        with torch.no_grad():
            feat = render_features(pkg["render"], gmap._obj_prob.detach())
        g = label_loss_grads(feat, target)
        rows = gmap._obj_prob
        rows.grad = self.last_grad = features_backward(tables, g.d_feat, gmap.nr_objects)
        gmap.object_optimizer.step()
        self.steps += 1
        return g.loss

    def run(self, viewpoints: Sequence, iters: int):
        """``iters`` steps cycling over ``viewpoints``; returns ``(first loss, last loss)`` as floats (ONE read-back, at the end)."""
        viewpoints = list(viewpoints)
        if not viewpoints or iters <= 0:
            return None, None
        for vp in viewpoints:
            self.target(vp)
        first = last = None
        for i in range(int(iters)):
            last = self.step(viewpoints[i % len(viewpoints)])
            if first is None:
                first = last
        a, b = torch.stack((first, last)).tolist()
        return float(a), float(b)


@torch.no_grad()
def render_labels(vp, intr, gmap, bg, min_opacity: float = 0.5):
    """``(feat [K, H, W], labels [H, W] int32)`` of the map's raw rows from ``vp``: one forward with detached geometry, one
    feature render.  The label is the argmax of the blended logits -- the class the label loss trains -- and -1 where the
    render's opacity is below ``min_opacity``."""
    from .feature_render import render_features
    with torch.enable_grad():
        _, pkg = _forward_tables(vp, intr, _frozen_geometry(gmap), bg)
    return render_features(pkg["render"], gmap._obj_prob.detach(), want_labels=True, min_opacity=min_opacity)


@torch.no_grad()
def eval_segmentation(frames: Sequence, gmap, intr, bg, kf_indices: Sequence[int], interval: int = 5) -> Dict:
    """Label accuracy and IoU of the map's rendered labels against the frames' ``segmentation`` on the frames ``eval_rendering``
    looks at (``evaluation.eval_frame_indices``: every ``interval``-th frame that is no keyframe).  One confusion matrix on the
    device, ONE read-back; returns ``segmentation_scores`` of it plus ``frames``, ``unseen`` (counted pixels without a
    prediction), ``ignored`` (pixels not counted) and ``stats`` (``readbacks``, ``renders``)."""
    from .evaluation import eval_frame_indices
    if gmap.nr_objects is None:
        raise ValueError("eval_segmentation needs a map with an object layer")
    K = gmap.nr_objects
    idx = eval_frame_indices(len(frames), kf_indices, interval)
    out = dict(pixel_accuracy=float("nan"), miou=float("nan"), iou=[float("nan")] * K, classes=0, frames=idx, unseen=0, ignored=0,
               stats=dict(readbacks=0, renders=0))
    if idx and len(gmap):
        acc = None
        geometry = _frozen_geometry(gmap)
        rows = gmap._obj_prob.detach()
        from .feature_render import render_features
        for i in idx:
            target = _target_of(frames[i])
            with torch.enable_grad():
                _, pkg = _forward_tables(frames[i], intr, geometry, bg)
            _, labels = render_features(pkg["render"], rows, want_labels=True)
            acc = label_confusion(labels, target, K, out=acc)
            out["stats"]["renders"] += 1
        both = torch.cat((acc[0].reshape(-1), acc[1])).cpu().numpy().view(np.uint32)       # the ONE read-back
        out["stats"]["readbacks"] += 1
        out.update(segmentation_scores(both[:K * K].reshape(K, K)), unseen=int(both[K * K]), ignored=int(both[K * K + 1]))
    return out
