"""The frame types of the package: ``Intrinsics`` and ``Viewpoint``, duck-typed stand-ins for the reference's CameraIntrinsics /
CameraExtrinsics (/root/reference/utils/camera_utils.py:8-79,82-221), the Scharr edge mask a viewpoint computes for itself
and the position error of a viewpoint against its ground-truth pose.  The dataset readers, the synthetic sequences, the tracker
and the run loops all build on these; nothing here measures anything."""
from __future__ import annotations

import math

import torch

from . import camera as cam


class Intrinsics:
    """``learnable=True``: the object owns ``delta``, a zero ``nn.Parameter`` of four floats that ``render()`` hands to the rasteriser
    as ``intr`` -- its ``.grad`` receives dL/d(fx, fy, cx, cy) -- and ``set`` moves the intrinsics (``calibration.IntrinsicsAdam``)."""

    def __init__(self, k: dict, device, learnable: bool = False):
        self.device = device
        self.height, self.width = k["H"], k["W"]
        self._build(dict(k))
        if learnable:
            self.delta = torch.nn.Parameter(torch.zeros(4, dtype=torch.float32, device=device))

    def _build(self, k: dict):
        self.k = k
        self.fx, self.fy, self.cx, self.cy = k["fx"], k["fy"], k["cx"], k["cy"]
        m = cam.camera_matrices(torch.eye(3), torch.zeros(3), k["fx"], k["fy"], k["cx"], k["cy"], k["W"], k["H"])
        self.projection_matrix = m.projmatrix_raw.to(self.device)   # transposed, as the reference's property
        self.FoVx, self.FoVy = 2 * math.atan(m.tanfovx), 2 * math.atan(m.tanfovy)

    def set(self, fx, fy, cx, cy):
        """New pinhole numbers: ``fx, fy, cx, cy``, ``k``, ``FoVx / FoVy`` and ``projection_matrix`` are rebuilt exactly as
        ``Intrinsics(new_k)`` builds them.  The matrix is a NEW tensor object, so every viewpoint's ``cached_camera_tensors``
        entry (keyed on the object) misses at its next render."""
        self._build(dict(self.k, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy)))


def scharr_grad_mask(rgb: torch.Tensor, edge_threshold: float = 1.1, eps: float = 0.01) -> torch.Tensor:
    """``CameraExtrinsics.compute_grad_mask`` (/root/reference/utils/camera_utils.py:185-216): Scharr gradient of the grey
    image (``image_gradient``, utils/slam_utils.py:6-23: reflect padding, normalised by 32), zeroed where a 3x3
    neighbourhood holds a pixel <= ``eps`` (``image_gradient_mask``, :26-40), thresholded at ``edge_threshold`` x median."""
    gray = rgb.mean(dim=0, keepdim=True)
    kx = torch.tensor([[3.0, 10.0, 3.0], [0.0, 0.0, 0.0], [-3.0, -10.0, -3.0]], device=rgb.device)
    ky = torch.tensor([[3.0, 0.0, -3.0], [10.0, 0.0, -10.0], [3.0, 0.0, -3.0]], device=rgb.device)
    pad = torch.nn.functional.pad(gray[None], (1, 1, 1, 1), mode="reflect")
    conv = torch.nn.functional.conv2d
    gv = conv(pad, kx.view(1, 1, 3, 3))[0] / 32.0
    gh = conv(pad, ky.view(1, 1, 3, 3))[0] / 32.0
    full = conv((pad.abs() > eps).float(), torch.ones(1, 1, 3, 3, device=rgb.device))[0] == 9.0
    mag = torch.sqrt((gv * full) ** 2 + (gh * full) ** 2)[0]
    return mag > mag.median() * edge_threshold


class Viewpoint:
    """``sensor="monocular"``: a frame without measured depth.  Its ``depth`` is an all-zero image -- the datasets' own "no
    measurement here" value, which keeps ``ones_like(depth)`` consumers working; pass one to share a single storage among the
    frames of a sequence, or None -- and its ``mask`` is and-ed with ``monocular.valid_rgb(rgb, rgb_boundary_threshold)``.  The
    tracker and the mapper pick the RGB-only losses for it (``fused_losses``)."""

    def __init__(self, idx, rgb, depth, device, gt_R=None, gt_T=None, mask=None, grad_mask=None, segmentation=None,
                 sensor="depth", rgb_boundary_threshold=0.01):
        if sensor not in ("depth", "monocular"):
            raise ValueError('sensor must be "depth" or "monocular"')
        self.frame_idx, self.device, self.sensor = idx, device, sensor
        if sensor == "monocular" and depth is None:
            depth = torch.zeros(rgb.shape[-2:], dtype=torch.float32, device=rgb.device)
        if segmentation is not None:        # [H,W] integer object ids: what the back-projection labels its points with
            self.segmentation = segmentation
        self.R = torch.eye(3, device=device)
        self.T = torch.zeros(3, device=device)
        self.R_gt, self.T_gt = gt_R, gt_T
        self.rgb, self.depth = rgb, depth
        # (a dataset frame brings both from monogs_amd.frame_ingest; the synthetic generators bring neither)
        self.mask = torch.ones_like(depth, dtype=torch.bool) if mask is None else mask
        if sensor == "monocular":
            self.mask = self.mask.bool() & (rgb.sum(dim=0) > rgb_boundary_threshold)      # (monocular.valid_rgb)
        self.grad_mask = scharr_grad_mask(rgb) if grad_mask is None else grad_mask
        z = lambda n, v=0.0: torch.nn.Parameter(torch.full((n,), v, device=device))  # noqa: E731
        self.cam_rot_delta, self.cam_trans_delta = z(3), z(3)
        self.exposure_a, self.exposure_b = z(1), z(1)

    @property
    def world_view_transform(self):
        return cam.world2view(self.R, self.T).transpose(0, 1)

    @property
    def camera_center(self):
        return self.world_view_transform.inverse()[3, :3]

    def update_RT(self, R, t):
        self.R, self.T = R.to(self.device).contiguous(), t.to(self.device).contiguous()

    def retract(self, thr=1e-4) -> bool:
        """update_pose (/root/reference/utils/pose_utils.py:76-93) on device tensors."""
        tau = torch.cat([self.cam_trans_delta.data, self.cam_rot_delta.data])
        Tm = torch.eye(4, device=self.device)
        Tm[:3, :3], Tm[:3, 3] = self.R, self.T
        Tn = cam.se3_exp(tau) @ Tm
        self.R, self.T = Tn[:3, :3], Tn[:3, 3]
        conv = bool(tau.norm() < thr)
        self.cam_rot_delta.data.zero_()
        self.cam_trans_delta.data.zero_()
        return conv


def mask_objects(vp: Viewpoint, ids, keep: bool = False, border: int = 0) -> Viewpoint:
    """A new ``Viewpoint`` of the same frame that does not look at the objects ``ids`` of ``vp.segmentation`` -- what the camera of a
    dynamic scene is tracked on: its ``mask`` excludes their pixels and its depth is zero there -- or, with ``keep=True``, that
    looks at nothing else (what the objects are tracked on).  ``border``: the pixels within that many pixels of the boundary between
    the objects and the rest are dropped as well (a render mixes the two sides of a silhouette; DESIGN.md, "Object motion").  Pose,
    exposure, ground truth, edge mask and segmentation are carried over; ``vp`` itself is untouched."""
    seg = getattr(vp, "segmentation", None)
    if seg is None:
        raise ValueError(f"frame {getattr(vp, 'frame_idx', '?')} carries no segmentation")
    hit = torch.isin(seg, torch.as_tensor([int(i) for i in ids], dtype=seg.dtype, device=seg.device))
    sel = hit if keep else ~hit
    if border > 0:            # erode what is kept: a pixel stays when its (2 border + 1)^2 neighbourhood holds nothing of the other side
        other = torch.nn.functional.max_pool2d((~sel)[None, None].float(), 2 * int(border) + 1, stride=1, padding=int(border))[0, 0]
        sel = other < 0.5
    out = Viewpoint(vp.frame_idx, vp.rgb, torch.where(sel, vp.depth, torch.zeros_like(vp.depth)), vp.device, gt_R=vp.R_gt, gt_T=vp.T_gt,
                    mask=vp.mask.bool() & sel, grad_mask=vp.grad_mask, segmentation=seg, sensor=vp.sensor)
    out.update_RT(vp.R.clone(), vp.T.clone())
    with torch.no_grad():
        out.exposure_a.copy_(vp.exposure_a); out.exposure_b.copy_(vp.exposure_b)
    return out


def position_error(vp) -> torch.Tensor:
    """Distance between the camera centre of ``vp``'s pose and that of its ground-truth pose (0-d tensor, metres)."""
    return (-(vp.R.t() @ vp.T) + (vp.R_gt.t() @ vp.T_gt)).norm()
