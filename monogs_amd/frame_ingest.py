"""From a decoded frame to what the tracker is handed, in one fused device path.

``MonocularDataset.__getitem__`` (/root/reference/utils/dataset.py:410-508) undistorts the colour image with ``cv2.remap``,
divides by 255, permutes, casts and uploads; ``CameraExtrinsics.compute_grad_mask`` (/root/reference/utils/camera_utils.py:184-212)
then runs a pad, three convolutions, a dozen elementwise operations and a ``torch.median`` that sorts the image.  Here the host
uploads the decoded 8-bit / 16-bit arrays as they are and ``mgs_frame_prepare`` (csrc/ingest.hip) does the rest in nine
launches: one preparation, one gradient intensity, the six of ``mgs_masked_median``, one threshold.

cv2 is not available to this project.  ``undistort_map`` restates ``cv2.initUndistortRectifyMap(K, dist, I, K)`` and the kernel
restates the fixed-point arithmetic of an 8-bit ``cv2.remap(INTER_LINEAR)`` from their documentation: parity with cv2 is
unpinned (the kernel is bit-exact against an integer mirror, tests/ingest_mirror.py).  Depth and segmentation are not
remapped: the reference undistorts the colour image only (dataset.py:452-453).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._launch import _device_guard, _stream

EDGE_THRESHOLD = 1.1      # camera_utils.py:185
GRAD_EPS = 0.01           # slam_utils.py:26


def undistort_map(fx, fy, cx, cy, k1, k2, p1, p2, k3, width, height) -> Tuple[np.ndarray, np.ndarray]:
    """``(map_x, map_y)``, float32 ``[height, width]``: for every pixel of the undistorted image, where to sample the distorted
    one -- ``initUndistortRectifyMap`` with R = I and the new camera matrix equal to K (dataset.py:335-342), in float64."""
    u, v = np.meshgrid(np.arange(int(width), dtype=np.float64), np.arange(int(height), dtype=np.float64))
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    kr = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


def masked_id_words(masked_ids: Iterable[int]) -> Tuple[int, ...]:
    """The 256-bit set ``mgs_frame_prepare`` takes: bit ``id & 31`` of word ``id >> 5``."""
    words = [0] * 8
    for i in masked_ids:
        if int(i) != i or not 0 <= int(i) <= 255:
            raise ValueError(f"masked id {i!r} is outside 0..255 (segmentation ids are 8-bit)")
        words[int(i) >> 5] |= 1 << (int(i) & 31)
    return tuple(words)


def _host_array(a, what: str) -> np.ndarray:
    if torch.is_tensor(a):
        if a.device.type != "cpu":
            raise ValueError(f"{what} must be a numpy array or a CPU tensor (got a tensor on {a.device})")
        a = a.numpy()
    if not isinstance(a, np.ndarray):
        raise ValueError(f"{what} must be a numpy array or a CPU tensor (got {type(a).__name__})")
    return a


def validate_frame(width: int, height: int, rgb_u8, depth_u16=None, segmentation=None):
    """The host-side checks of ``FrameIngest.prepare``; touches no device.  Returns C-contiguous numpy arrays
    ``(uint8 [H,W,3], uint16 [H,W] or None, uint8 [H,W] or None)``.  Depth may come in any integer type (PIL decodes a 16-bit
    PNG as uint16 or as int32, depending on its mode) as long as every value fits 16 bits."""
    rgb = _host_array(rgb_u8, "rgb_u8")
    if rgb.dtype != np.uint8:
        raise ValueError(f"rgb_u8 must be uint8 (got {rgb.dtype})")
    if rgb.shape != (height, width, 3):
        raise ValueError(f"rgb_u8 must be [{height}, {width}, 3] (got {list(rgb.shape)})")
    depth = seg = None
    if depth_u16 is not None:
        depth = _host_array(depth_u16, "depth_u16")
        if depth.dtype.kind not in "iu":
            raise ValueError(f"depth_u16 must be an integer array (got {depth.dtype})")
        if depth.shape != (height, width):
            raise ValueError(f"depth_u16 must be [{height}, {width}] (got {list(depth.shape)})")
        if depth.dtype != np.uint16:
            if depth.size and (int(depth.min()) < 0 or int(depth.max()) > 65535):
                raise ValueError("depth_u16 holds a value that does not fit 16 bits")
            depth = depth.astype(np.uint16)
    if segmentation is not None:
        seg = _host_array(segmentation, "segmentation")
        if seg.dtype != np.uint8:
            raise ValueError(f"segmentation must be uint8 (got {seg.dtype})")
        if seg.shape != (height, width):
            raise ValueError(f"segmentation must be [{height}, {width}] (got {list(seg.shape)})")
    c = np.ascontiguousarray
    return c(rgb), None if depth is None else c(depth), None if seg is None else c(seg)


def _require_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: no CPU path (the ingest kernels are HIP only)")


def grad_mask_scratch(width: int, height: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().mgs_grad_mask_scratch_bytes(int(width), int(height)), dtype=torch.uint8, device=device)


@torch.no_grad()
def grad_mask(rgb: torch.Tensor, edge_threshold: float = EDGE_THRESHOLD, eps: float = GRAD_EPS,
              scratch: Optional[torch.Tensor] = None, return_intensity: bool = False):
    """``compute_grad_mask`` of a ``[3,H,W]`` float32 device image through ``mgs_grad_mask``: a drop-in for
    ``frames.scharr_grad_mask`` (bool ``[H,W]``), eight launches, no host synchronisation.  With ``return_intensity`` the
    pair ``(grad_mask, intensity)``."""
    _require_device(rgb, "grad_mask")
    if rgb.dim() != 3 or rgb.shape[0] != 3 or rgb.dtype != torch.float32:
        raise ValueError(f"grad_mask takes a float32 [3,H,W] image (got {rgb.dtype} {tuple(rgb.shape)})")
    rgb = rgb.detach().contiguous()
    H, W = int(rgb.shape[1]), int(rgb.shape[2])
    dev = rgb.device
    if scratch is None:
        scratch = grad_mask_scratch(W, H, dev)
    out = torch.empty(H, W, dtype=torch.uint8, device=dev)
    intensity = torch.empty(H, W, dtype=torch.float32, device=dev) if return_intensity else None
    with _device_guard(dev):
        _lib.check(_lib.load().mgs_grad_mask(W, H, rgb.data_ptr(), float(edge_threshold), float(eps), scratch.data_ptr(),
                                             out.data_ptr(), None if intensity is None else intensity.data_ptr(), _stream()),
                   "mgs_grad_mask")
    mask = out.view(torch.bool)
    return (mask, intensity) if return_intensity else mask


class FrameIngest:
    """The device half of the dataset for one image size.  Owns the undistortion maps (when ``calibration["distorted"]``), the
    scratch of ``mgs_frame_prepare``, and one frame's pinned staging and device input buffers.  Nothing touches the device
    before the first ``prepare`` has validated its arguments."""

    def __init__(self, width: int, height: int, calibration: dict, device, masked_ids: Iterable[int] = ()):
        self.width, self.height = int(width), int(height)
        if self.width < 2 or self.height < 2:
            raise ValueError("FrameIngest needs an image of at least 2 x 2 pixels")
        self.device = torch.device(device)
        self.masked_words = masked_id_words(masked_ids)
        self.depth_scale = float(calibration.get("depth_scale") or 1.0)
        self.distorted = bool(calibration.get("distorted", False))
        self.host_maps = None
        if self.distorted:
            self.host_maps = undistort_map(*(float(calibration[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")),
                                           self.width, self.height)
        self._ready = False

    def _allocate(self):
        H, W, dev = self.height, self.width, self.device
        if dev.type != "cuda":
            raise RuntimeError("FrameIngest: no CPU path (the ingest kernels are HIP only)")
        self.map_x = self.map_y = None
        if self.host_maps is not None:
            self.map_x, self.map_y = (torch.from_numpy(m).to(dev) for m in self.host_maps)
        self.scratch = grad_mask_scratch(W, H, dev)
        pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()      # noqa: E731
        self._pin = dict(rgb=pin((H, W, 3), torch.uint8), depth=pin((H, W), torch.uint16), seg=pin((H, W), torch.uint8))
        self._in = dict(rgb=torch.empty(H, W, 3, dtype=torch.uint8, device=dev),
                        depth=torch.empty(H, W, dtype=torch.uint16, device=dev),
                        seg=torch.empty(H, W, dtype=torch.uint8, device=dev))
        self._uploaded = torch.cuda.Event()
        self._ready = True

    def static_inputs(self) -> Dict[str, torch.Tensor]:
        """The device input buffers ``prepare`` uploads into (``rgb`` uint8 [H,W,3], ``depth`` uint16 [H,W], ``seg`` uint8
        [H,W]): what a captured ``prepare_device`` reads on replay."""
        if not self._ready:
            self._allocate()
        return self._in

    @torch.no_grad()
    def prepare_device(self, rgb_u8: torch.Tensor, depth_u16: Optional[torch.Tensor] = None,
                       segmentation: Optional[torch.Tensor] = None, want_intensity: bool = False) -> Dict[str, torch.Tensor]:
        """``mgs_frame_prepare`` on device tensors, on the current stream: nine launches into fresh outputs, no host
        synchronisation, capturable.  Returns ``rgb`` float32 [3,H,W], ``depth`` float32 [H,W] or None, ``mask`` and
        ``grad_mask`` bool [H,W] and, when asked for, ``intensity`` float32 [H,W]."""
        if not self._ready:
            self._allocate()
        H, W, dev = self.height, self.width, self.device
        for t, dt, shape, what in ((rgb_u8, torch.uint8, (H, W, 3), "rgb_u8"), (depth_u16, torch.uint16, (H, W), "depth_u16"),
                                   (segmentation, torch.uint8, (H, W), "segmentation")):
            if t is not None and (t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{what} must be a contiguous {dt} tensor of shape {list(shape)} on {dev}")
        p = _lib.MgsFramePrepare()
        p.width, p.height = W, H
        p.rgb_u8 = rgb_u8.data_ptr()
        if self.map_x is not None:
            p.map_x, p.map_y = self.map_x.data_ptr(), self.map_y.data_ptr()
        rgb = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
        gmask = torch.empty(H, W, dtype=torch.uint8, device=dev)
        depth = intensity = None
        if depth_u16 is not None:
            depth = torch.empty(H, W, dtype=torch.float32, device=dev)
            p.depth_u16, p.depth_out, p.depth_scale = depth_u16.data_ptr(), depth.data_ptr(), self.depth_scale
        if segmentation is not None:
            p.segmentation = segmentation.data_ptr()
        if want_intensity:
            intensity = torch.empty(H, W, dtype=torch.float32, device=dev)
            p.intensity_out = intensity.data_ptr()
        p.masked_ids = (C.c_uint32 * 8)(*self.masked_words)
        p.rgb_out, p.mask_out, p.grad_mask_out = rgb.data_ptr(), mask.data_ptr(), gmask.data_ptr()
        p.edge_threshold, p.eps = EDGE_THRESHOLD, GRAD_EPS
        p.scratch = self.scratch.data_ptr()
        with _device_guard(dev):
            _lib.check(_lib.load().mgs_frame_prepare(C.byref(p), _stream()), "mgs_frame_prepare")
        out = dict(rgb=rgb, depth=depth, mask=mask.view(torch.bool), grad_mask=gmask.view(torch.bool))
        if want_intensity:
            out["intensity"] = intensity
        return out

    def prepare(self, rgb_u8, depth_u16=None, segmentation=None) -> Dict[str, Optional[torch.Tensor]]:
        """One decoded frame (numpy arrays or CPU tensors: uint8 [H,W,3], 16-bit [H,W], uint8 ids [H,W]) -> the reference's
        ``data`` dict without the pose, plus ``grad_mask``: ``rgb`` float32 [3,H,W], ``depth`` float32 [H,W] or None, ``mask``
        bool, ``segmentation`` long or None, ``grad_mask`` bool.  A wrong dtype or shape, or a depth value beyond 16 bits,
        raises ``ValueError`` before the device is touched."""
        rgb, depth, seg = validate_frame(self.width, self.height, rgb_u8, depth_u16, segmentation)
        if not self._ready:
            self._allocate()
        with _device_guard(self.device):
            self._uploaded.synchronize()                  # the previous frame's copies have left the pinned buffers
            given = {}
            for key, a in (("rgb", rgb), ("depth", depth), ("seg", seg)):
                if a is not None:
                    self._pin[key].numpy()[...] = a
                    self._in[key].copy_(self._pin[key], non_blocking=True)
                    given[key] = self._in[key]
            self._uploaded.record()
            out = self.prepare_device(given["rgb"], given.get("depth"), given.get("seg"))
            out["segmentation"] = given["seg"].to(torch.long) if seg is not None else None
        return out
