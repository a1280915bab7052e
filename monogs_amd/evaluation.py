"""Render and trajectory evaluation: ``eval_rendering`` / ``eval_traj_ate`` of /root/reference/utils/eval_utils.py:26-208.

``eval_rendering``: PSNR over ``gt > 0`` and SSIM of the clamped render on every ``interval``-th frame that is not a keyframe,
one no-grad render + ``mgs_image_metrics`` + ``mgs_ssim_forward`` per frame into one device table, ONE read-back at the end.
``eval_ate``: absolute trajectory error of the camera centres, optionally after the Umeyama alignment the reference intends
(float64 numpy on the host: a few hundred 3-vectors).  What stays out: LPIPS (AlexNet weights), the plots and wandb.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._launch import _f32, _stream, _device_guard
from .ssim import C1 as SSIM_C1, C2 as SSIM_C2


# ---- image metrics ---------------------------------------------------------------------------------------------------------
class _MetricsScratch:
    """The two scratch buffers of one image size, allocated once per evaluation."""

    def __init__(self, W: int, H: int, device):
        lib = _lib.load()
        self.metrics = torch.empty(lib.mgs_metrics_scratch_bytes(W, H), dtype=torch.uint8, device=device)
        self.ssim = torch.empty(lib.mgs_ssim_scratch_bytes(3, W, H, 0) // 4, dtype=torch.float32, device=device)


@torch.no_grad()
def image_metrics(render: torch.Tensor, gt: torch.Tensor, row: Optional[torch.Tensor] = None, want_u8: bool = False,
                  clamped_out: Optional[torch.Tensor] = None, scratch: Optional[_MetricsScratch] = None):
    """One frame of ``eval_rendering`` (eval_utils.py:169-183) in four launches and no host synchronisation:
    ``row`` (device float[4], allocated when None) = ``{psnr over gt > 0, ssim(clamp(render), gt), mse, count}``.
    Returns ``(row, clamped [3,H,W], u8 [H,W,3] or None)``.  ``render`` / ``gt``: [3,H,W] float32 on the device, at least 11 x 11
    (the SSIM window); views that start inside a larger buffer are taken as they are (the kernel has a scalar path for them)."""
    lib = _lib.load()
    if render.dim() != 3 or render.shape[0] != 3 or render.shape != gt.shape:
        raise ValueError(f"image_metrics takes two [3,H,W] images (got {tuple(render.shape)} and {tuple(gt.shape)})")
    render, gt = _f32(render.detach(), "render"), _f32(gt.detach(), "gt")
    H, W = int(render.shape[1]), int(render.shape[2])
    dev = render.device
    if clamped_out is None:
        clamped_out = torch.empty_like(render)
    elif clamped_out.shape != render.shape or clamped_out.dtype != torch.float32 or not clamped_out.is_contiguous():
        raise ValueError("clamped_out must be a contiguous float32 tensor of the render's shape")
    if row is None:
        row = torch.empty(4, dtype=torch.float32, device=dev)
    elif row.dtype != torch.float32 or row.numel() != 4 or not row.is_contiguous():
        raise ValueError("row must be a contiguous float32 tensor of 4 elements")
    u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    sc = scratch if scratch is not None else _MetricsScratch(W, H, dev)
    with _device_guard(dev):
        _lib.check(lib.mgs_image_metrics(W, H, render.data_ptr(), gt.data_ptr(), clamped_out.data_ptr(),
                                         None if u8 is None else u8.data_ptr(), sc.metrics.data_ptr(), row.data_ptr(), _stream()),
                   "mgs_image_metrics")
        _lib.check(lib.mgs_ssim_forward(3, W, H, 1, 0, SSIM_C1, SSIM_C2, clamped_out.data_ptr(), gt.data_ptr(),
                                        sc.ssim.data_ptr(), row.data_ptr() + 4, _stream()), "mgs_ssim_forward")
    return row, clamped_out, u8


def eval_frame_indices(n_frames: int, kf_indices: Sequence[int], interval: int = 5) -> List[int]:
    """The frames ``eval_rendering`` looks at (eval_utils.py:144-154): ``range(0, n_frames - 1, interval)`` without the
    keyframes.  (The reference's ``end_idx`` expression -- ``... if iteration == "final" or "before_opt" else iteration`` -- always
    takes its first branch.)"""
    kf = set(int(k) for k in kf_indices)
    return [i for i in range(0, int(n_frames) - 1, int(interval)) if i not in kf]


@torch.no_grad()
def eval_rendering(frames: Sequence, gmap, intr, bg, kf_indices: Sequence[int], interval: int = 5, save_dir: Optional[str] = None,
                   tag: str = "final") -> Dict:
    """``eval_rendering`` of the reference (eval_utils.py:131-208) over ``frames`` (objects with ``R``, ``T``, ``rgb`` and the
    zero pose deltas ``render()`` takes): ``mean_psnr``, ``mean_ssim``, ``frames`` (the indices evaluated), ``per_frame`` and
    ``stats`` (``readbacks``: result read-backs, one).  The ground truth is the frame's own ``rgb``.  ``mean_lpips`` is
    OMITTED: LPIPS needs the AlexNet weights of torchmetrics, which this project does not ship.  With ``save_dir`` the three
    means go to ``<save_dir>/psnr/<tag>/final_result.json`` as the reference writes them."""
    from .gaussian_optim import activate
    from .renderer import render
    idx = eval_frame_indices(len(frames), kf_indices, interval)
    out = dict(mean_psnr=float("nan"), mean_ssim=float("nan"), frames=idx, per_frame=[], stats=dict(readbacks=0, renders=0))
    if idx and len(gmap):
        dev = gmap.device
        H, W = int(intr.height), int(intr.width)
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
        xyz, feat = gmap._xyz.detach(), gmap._rgb.detach()
        table = torch.empty(len(idx), 4, dtype=torch.float32, device=dev)
        clamped = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        sc = _MetricsScratch(W, H, dev)
        for j, i in enumerate(idx):
            image = render(frames[i], intr, xyz, rot, scales3, opac, feat, bg)["render"]
            image_metrics(image, frames[i].rgb, row=table[j], clamped_out=clamped, scratch=sc)
            out["stats"]["renders"] += 1
        rows = table.cpu().double().numpy()                       # the ONE read-back
        out["stats"]["readbacks"] += 1
        out["per_frame"] = [dict(frame=i, psnr=float(r[0]), ssim=float(r[1]), mse=float(r[2]), count=int(r[3])) for i, r in zip(idx, rows)]
        out["mean_psnr"], out["mean_ssim"] = float(np.mean(rows[:, 0])), float(np.mean(rows[:, 1]))
    if save_dir is not None:
        d = os.path.join(save_dir, "psnr", str(tag))
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "final_result.json"), "w", encoding="utf-8") as f:
            json.dump(dict(mean_psnr=out["mean_psnr"], mean_ssim=out["mean_ssim"]), f, indent=4)
    return out


# ---- trajectory -----------------------------------------------------------------------------------------------------------
def _np(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _camera_centre(R, T):
    """Translation of the camera-to-world matrix, formed as the reference does: ``np.linalg.inv`` of the 4x4 (eval_utils.py:34-67)."""
    pose = np.eye(4)
    pose[0:3, 0:3] = _np(R)
    pose[0:3, 3] = _np(T)
    return np.linalg.inv(pose)[0:3, 3]


def umeyama(x: np.ndarray, y: np.ndarray, with_scale: bool):
    """Least-squares ``(R, t, c)`` with ``y ~ c R x + t`` for two [n,3] point sets (Umeyama 1991, eqs. 34-43), ``c = 1`` unless
    ``with_scale``; det(R) = +1 always (the reflection fix of eq. 39/43).  Fewer than two distinct points: R = I, c = 1."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[0]
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    var_x = float((xc ** 2).sum() / n)
    if n < 2 or var_x == 0.0:
        return np.eye(3), my - mx, 1.0
    cov = yc.T @ xc / n
    U, d, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    c = float(np.trace(np.diag(d) @ S) / var_x) if (with_scale and var_x > 0.0) else 1.0
    t = my - c * R @ mx
    return R, t, c


def eval_ate(frames: Sequence, kf_ids: Optional[Sequence[int]] = None, align: bool = False, correct_scale: bool = False) -> Dict:
    """Absolute trajectory error of ``eval_traj_ate`` (eval_utils.py:26-128) over ``frames[k] for k in kf_ids`` (default: every
    frame): translation part of estimated against ground-truth camera-to-world poses (``R``, ``T`` / ``R_gt``, ``T_gt`` are
    world-to-camera, inverted as there).  Returns ``rmse``, ``mean``, ``median``, ``min``, ``max`` and ``n``.
    ``align=False`` is what the reference actually reports: it aligns a copy and then overwrites it with the unaligned
    trajectory (:88-92).  ``align=True`` is the alignment it intends: Umeyama of the estimate onto the ground truth, rigid, or a
    similarity with ``correct_scale``.  Parity with ``evo`` is unpinned: the package is not a dependency of this project."""
    ids = list(range(len(frames))) if kf_ids is None else [int(k) for k in kf_ids]
    if not ids:
        return dict(rmse=float("inf"), n=0)            # the reference returns np.inf without ground-truth poses
    est = np.stack([_camera_centre(frames[k].R, frames[k].T) for k in ids])
    gt = np.stack([_camera_centre(frames[k].R_gt, frames[k].T_gt) for k in ids])
    if align:
        R, t, c = umeyama(est, gt, with_scale=correct_scale)
        est = c * est @ R.T + t
    e = np.linalg.norm(gt - est, axis=1)
    return dict(rmse=float(np.sqrt(np.mean(e ** 2))), mean=float(np.mean(e)), median=float(np.median(e)), min=float(np.min(e)),
                max=float(np.max(e)), n=len(ids), aligned=bool(align),
                correct_scale=bool(align and correct_scale))
