"""Camera-matrix and pose helpers on the caller's side of the rasteriser boundary.

These mirror the conventions of the reference's helpers so that the tensors handed to
``GaussianRasterizationSettings`` are the same ones MonoGS builds:

* ``world2view`` / ``projection_matrix`` / ``full_proj_transform``:
  /root/reference/gaussian_splatting/utils/graphics_utils.py:33-42,68-89 and
  /root/reference/utils/camera_utils.py:39-49,171-178,224-231.  All three matrices are handed to
  the kernels TRANSPOSED (row-vector convention): flat element ``4*j+i`` of the tensor is maths
  element (i, j).
* ``se3_exp`` / ``retract_pose``: /root/reference/utils/pose_utils.py:25-93 --
  ``T_cw <- exp([rho; theta]^) @ T_cw``; this is the convention dL/dtheta and dL/drho of the
  rasteriser are defined against.

They are checked against values produced by the reference's own functions in
tests/test_golden.py (fixtures tests/golden/camera_pose.npz).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

ZNEAR = 0.01   # /root/reference/utils/camera_utils.py:41-42
ZFAR = 100.0


def world2view(R: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """4x4 world-to-camera matrix [[R, t], [0, 1]]; R, t are already world->camera."""
    M = torch.eye(4, dtype=torch.float32, device=R.device)     # (no host scalar writes: hipGraph-capturable)
    M[:3, :3] = R
    M[:3, 3] = t
    return M


def fused_camera_matrices(R: torch.Tensor, t: torch.Tensor, projmatrix_raw: torch.Tensor, out=None):
    """(viewmatrix, projmatrix, campos) -- the three transposed camera tensors of GaussianRasterizationSettings --
    from device tensors R[3,3], t[3] (world->camera) and the transposed projection, in one launch
    (``mgs_camera_setup``).  Same values as ``world2view(R, t).T``, ``viewmatrix @ projmatrix_raw`` and
    ``viewmatrix.inverse()[3, :3]``; no autograd (the pose and the intrinsics take their gradients through the rasteriser's
    ``theta`` / ``rho`` / ``intr`` holders, not through these tensors).
    ``out``: three existing tensors to write into (a loop whose pose step keeps them current -- ``PoseAdam.step_and_retract(camera=...)`` --
    computes them once per frame, not once per render)."""
    from . import _lib
    from ._launch import _stream, _device_guard
    lib = _lib.load()
    f = lambda x: x.detach().to(torch.float32).contiguous()  # noqa: E731
    R, t, Pm = f(R), f(t), f(projmatrix_raw)
    dev = R.device
    if out is not None:
        view, full, campos = out
    else:
        view = torch.empty(4, 4, dtype=torch.float32, device=dev)
        full = torch.empty(4, 4, dtype=torch.float32, device=dev)
        campos = torch.empty(3, dtype=torch.float32, device=dev)
    with _device_guard(dev):
        _lib.check(lib.mgs_camera_setup(R.data_ptr(), t.data_ptr(), Pm.data_ptr(), view.data_ptr(), full.data_ptr(),
                                        campos.data_ptr(), _stream()), "mgs_camera_setup")
    return view, full, campos


def cached_camera_tensors(viewpoint, R: torch.Tensor, t: torch.Tensor, projmatrix_raw: torch.Tensor):
    """``fused_camera_matrices`` remembered on the viewpoint object: recomputed only when ``R``, ``t`` or the projection
    are different tensor OBJECTS from the ones the cache was made from (``update_RT`` assigns new tensors, as the
    reference's ``Camera.update_RT`` does, utils/camera_utils.py:165-167) or were edited in place by a torch op since
    (tensor version counters).  ``PoseAdam.step_and_retract`` updates
    R, t in place and rewrites the cached tensors in the same launch, so a mapping / tracking loop launches no camera
    kernel per render.  Falls back to a plain call for objects that take no new attributes."""
    c = getattr(viewpoint, "_mgs_cam", None)
    if (c is not None and c[0] is R and c[1] is t and c[2] is projmatrix_raw
            and c[4] == (R._version, t._version, projmatrix_raw._version)):
        return c[3]
    out = fused_camera_matrices(R, t, projmatrix_raw)
    ok = (R.dtype == torch.float32 and t.dtype == torch.float32 and projmatrix_raw.dtype == torch.float32
          and R.is_contiguous() and t.is_contiguous() and projmatrix_raw.is_contiguous())
    try:
        # (the version counters catch in-place torch edits of R / t; the fused pose step writes through raw pointers, bumps
        #  no counter and refreshes the cached tensors itself)
        viewpoint._mgs_cam = (R, t, projmatrix_raw, out, (R._version, t._version, projmatrix_raw._version)) if ok else None
    except AttributeError:
        pass
    return out


def projection_matrix(fx, fy, cx, cy, W, H, znear=ZNEAR, zfar=ZFAR, device="cpu") -> torch.Tensor:
    """Off-centre pinhole projection, z in [znear, zfar] -> [0, 1], w = z (un-transposed)."""
    fx_t = torch.as_tensor([float(fx)], dtype=torch.float32, device=device)
    fy_t = torch.as_tensor([float(fy)], dtype=torch.float32, device=device)
    # frustum edges on the near plane, computed in the same float32 steps as the reference
    l_ = znear / fx_t * (((2 * cx - W) / W - 1.0) * W / 2.0)
    r_ = znear / fx_t * (((2 * cx - W) / W + 1.0) * W / 2.0)
    t_ = znear / fy_t * (((2 * cy - H) / H + 1.0) * H / 2.0)
    b_ = znear / fy_t * (((2 * cy - H) / H - 1.0) * H / 2.0)
    Pm = torch.zeros(4, 4, dtype=torch.float32, device=device)
    Pm[0, 0] = 2.0 * znear / (r_ - l_)
    Pm[1, 1] = 2.0 * znear / (t_ - b_)
    Pm[0, 2] = (r_ + l_) / (r_ - l_)
    Pm[1, 2] = (t_ + b_) / (t_ - b_)
    Pm[3, 2] = 1.0
    Pm[2, 2] = zfar / (zfar - znear)
    Pm[2, 3] = -(zfar * znear) / (zfar - znear)
    return Pm


def _skew(v: torch.Tensor) -> torch.Tensor:
    S = torch.zeros(3, 3, dtype=v.dtype, device=v.device)
    S[0, 1], S[0, 2] = -v[2], v[1]
    S[1, 0], S[1, 2] = v[2], -v[0]
    S[2, 0], S[2, 1] = -v[1], v[0]
    return S


def so3_exp(theta: torch.Tensor) -> torch.Tensor:
    K = _skew(theta)
    K2 = K @ K
    a = torch.norm(theta)
    eye = torch.eye(3, dtype=theta.dtype, device=theta.device)
    if a < 1e-5:
        return eye + K + 0.5 * K2
    return eye + (torch.sin(a) / a) * K + ((1 - torch.cos(a)) / (a ** 2)) * K2


def so3_left_jacobian(theta: torch.Tensor) -> torch.Tensor:
    K = _skew(theta)
    K2 = K @ K
    a = torch.norm(theta)
    eye = torch.eye(3, dtype=theta.dtype, device=theta.device)
    if a < 1e-5:
        return eye + 0.5 * K + (1.0 / 6.0) * K2
    return eye + K * ((1.0 - torch.cos(a)) / (a ** 2)) + K2 * ((a - torch.sin(a)) / (a ** 3))


def se3_exp(tau: torch.Tensor) -> torch.Tensor:
    """tau = [rho; theta] -> 4x4."""
    T = torch.eye(4, dtype=tau.dtype, device=tau.device)
    T[:3, :3] = so3_exp(tau[3:])
    T[:3, 3] = so3_left_jacobian(tau[3:]) @ tau[:3]
    return T


def retract_pose(R: torch.Tensor, t: torch.Tensor, rho: torch.Tensor, theta: torch.Tensor,
                 converged_threshold: float = 1e-4):
    """Left-multiplicative update used after every optimiser step.  Returns (R', t', converged)."""
    tau = torch.cat([rho, theta])
    T = torch.eye(4, dtype=tau.dtype, device=tau.device)
    T[:3, :3] = R
    T[:3, 3] = t
    Tn = se3_exp(tau) @ T
    return Tn[:3, :3], Tn[:3, 3], bool(tau.norm() < converged_threshold)


class CameraMatrices(NamedTuple):
    viewmatrix: torch.Tensor       # [4,4] transposed world->camera
    projmatrix: torch.Tensor       # [4,4] transposed  P @ T_cw
    projmatrix_raw: torch.Tensor   # [4,4] transposed  P
    campos: torch.Tensor           # [3]
    tanfovx: float
    tanfovy: float


def camera_matrices(R, t, fx, fy, cx, cy, W, H, device="cpu") -> CameraMatrices:
    """Everything ``render()`` feeds into the settings tuple
    (/root/reference/gaussian_splatting/gaussian_renderer/__init__.py:62-84)."""
    view_t = world2view(R.to(device), t.to(device)).transpose(0, 1)
    proj_t = projection_matrix(fx, fy, cx, cy, W, H, device=device).transpose(0, 1)
    full_t = view_t.unsqueeze(0).bmm(proj_t.unsqueeze(0)).squeeze(0)
    campos = view_t.inverse()[3, :3]
    # float32 atan then a Python float, as /root/reference/utils/camera_utils.py:30-36 does
    fovx = 2 * torch.atan(W / (2 * torch.tensor([float(fx)], dtype=torch.float32))).item()
    fovy = 2 * torch.atan(H / (2 * torch.tensor([float(fy)], dtype=torch.float32))).item()
    return CameraMatrices(view_t.contiguous(), full_t.contiguous(), proj_t.contiguous(), campos.contiguous(),
                          math.tan(fovx * 0.5), math.tan(fovy * 0.5))


# intrinsics of the reference's configs used by BASELINE.json
INTRINSICS = {
    # /root/reference/configs/mono/tum/fr3_office.yaml:6-16
    "fr3_office": dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, W=640, H=480),
    # /root/reference/configs/rgbd/replica/base_config.yaml:17-28
    "replica": dict(fx=600.0, fy=600.0, cx=599.5, cy=339.5, W=1200, H=680),
    # /root/reference/configs/mono/davis/car-turn.yaml:5-18 (the only 1920x1080 config)
    "davis_1080p": dict(fx=960.0, fy=960.0, cx=960.0, cy=540.0, W=1920, H=1080),
}
