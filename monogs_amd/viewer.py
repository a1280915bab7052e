"""Headless viewer: the frames the reference's viewer window shows, as ``uint8 [H, W, 3]`` images on the device.

The reference's third process (viewer/slam_viewer.py) needs Open3D's GUI, GLFW and an OpenGL context and cannot run on a headless
server.  Here ``HeadlessViewer.frame(snapshot, camera, mode)`` renders what it would show for any free camera:

* ``rgb`` / ``segmentation`` / ``depth`` / ``time``: one rasteriser forward (``segmentation`` with ``palette[obj_idx]`` as the colour
  override, slam_viewer.py:700), converted to bytes by ``mgs_viewer_compose`` with the reference's own rules (:600-636, :767-768);
* ``elipsoids`` (the reference's spelling; its GL renderer with ``render_mod = -4``, gl_render/shaders/gau_frag.glsl:20-35): the
  nearest splat with alpha > 0.4 per pixel, ``mgs_viewer_ellipsoids`` through the scratch of that forward, which also gives the pick
  buffer (``want_hit=True``);
* keyframe frustums, the current and the ground-truth camera and the trajectory are drawn over the image without a depth test, as
  Open3D draws its line sets over the background image: the host clips and projects the segments in float64 and quantises them
  to 1/16 pixel, ``mgs_viewer_lines`` rasterises them with integer arithmetic (``tests/viewer_mirror.py`` restates the rule).

Nothing on the frame path reads back from the device.  The first frame of a (snapshot, camera) pair uploads the camera and the
segments; a repeated frame (a ``torch.cuda.graph`` capture, say) launches kernels only.  Parity with Open3D's line drawing, and
with the frustum colours beyond the ones quoted below, is unpinned.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .camera import fused_camera_matrices
from .gaussian_map import object_labels
from ._launch import _device_guard, _ptr, _stream
from .rasterizer import GaussianRasterizer, forward_scratch
from .renderer import raster_settings

MODES = ("rgb", "segmentation", "depth", "time", "elipsoids")
_COMPOSE_MODE = dict(rgb=_lib.H.MGS_VIEWER_RGB, segmentation=_lib.H.MGS_VIEWER_RGB, depth=_lib.H.MGS_VIEWER_DEPTH, time=_lib.H.MGS_VIEWER_TIME,
                     elipsoids=_lib.H.MGS_VIEWER_ELLIPSOIDS)
ELLIPSOID_THRESHOLD = 0.4            # gau_frag.glsl:30-33
NEAR = 0.2                           # the rasteriser's near plane: segments are clipped against z >= NEAR
GUARD = 1024.0                       # segments are clipped to the image grown by this many pixels before quantisation
SUBPIXEL = 16
# slam_viewer.py:456 (current: green), :484 (ground truth: red), :520 (keyframes of the window: yellow); the trajectory is ours
COLOR_CURRENT, COLOR_GT, COLOR_KEYFRAME, COLOR_TRAJECTORY = (0, 255, 0), (255, 0, 0), (255, 255, 0), (255, 255, 255)

# matplotlib's "jet" (its _jet_data): linear segments through these knots, sampled at i / 255
_JET_KNOTS = dict(
    red=((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    green=((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    blue=((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)))


def jet_lut() -> np.ndarray:
    """``uint8 [256, 3]``: ``trunc(lut * 255)`` of the 256-entry jet table, what the reference's ``color_map(x)[..., :3] * 255`` cast
    leaves.  Interpolated as matplotlib's ``_create_lookup_table`` does, in float64."""
    xind = 255 * np.linspace(0.0, 1.0, 256)          # (knots and sample positions both scaled by N - 1, as matplotlib rounds them)
    out = np.empty((256, 3), dtype=np.uint8)
    for c, name in enumerate(("red", "green", "blue")):
        k = np.array(_JET_KNOTS[name], dtype=np.float64)
        x, y = k[:, 0] * 255, k[:, 1]
        ind = np.searchsorted(x, xind)[1:-1]
        dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate([[y[0]], dist * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
        out[:, c] = np.clip(lut, 0.0, 1.0) * 255                              # (the cast truncates)
    return out


# ---- cameras (host side, float64) ------------------------------------------------------------------------------------------
def _np(x) -> np.ndarray:
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


class FreeCamera:
    """A world->camera pose ``(R, T)`` kept on the host in float64; its device tensors are made once, on first use."""

    def __init__(self, R, T):
        self.R, self.T = _np(R).reshape(3, 3), _np(T).reshape(3)
        self._dev = {}

    @classmethod
    def of(cls, cam) -> "FreeCamera":
        if isinstance(cam, FreeCamera):
            return cam
        if isinstance(cam, (tuple, list)):
            return cls(*cam)
        return cls(cam.R, cam.T)

    @property
    def c2w(self) -> np.ndarray:
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = self.R.T, -self.R.T @ self.T
        return M

    def tensors(self, intr):
        key = (str(intr.projection_matrix.device), intr.projection_matrix.data_ptr())
        if key not in self._dev:
            dev = intr.projection_matrix.device
            f = lambda a: torch.tensor(a, dtype=torch.float32).to(dev)  # noqa: E731
            self._dev[key] = fused_camera_matrices(f(self.R), f(self.T), intr.projection_matrix)
        return self._dev[key]


def look_at(eye, target, up) -> FreeCamera:
    """The camera at ``eye`` looking at ``target`` with ``up`` pointing up in the image (x right, y down, z forward)."""
    eye, target, up = _np(eye), _np(target), _np(up)
    f = target - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    if np.linalg.norm(r) < 1e-12:
        raise ValueError("look_at: up is parallel to the viewing direction")
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    return FreeCamera(R, -R @ eye)


def orbit(centre, radius: float, n: int, height: float = 0.0, up=(0.0, -1.0, 0.0)) -> list:
    """``n`` cameras on a circle of ``radius`` around ``centre`` in the plane orthogonal to ``up``, ``height`` along it, looking in."""
    centre, upv = _np(centre), _np(up)
    upv = upv / np.linalg.norm(upv)
    a = np.cross(upv, (1.0, 0.0, 0.0) if abs(upv[0]) < 0.9 else (0.0, 1.0, 0.0))
    a = a / np.linalg.norm(a)
    b = np.cross(upv, a)
    return [look_at(centre + radius * (math.cos(t) * a + math.sin(t) * b) + height * upv, centre, upv)
            for t in (2.0 * math.pi * i / n for i in range(int(n)))]


def frustum_points(c2w, intr, size: float = 1.0) -> np.ndarray:
    """World-space ``[5, 3]``: the apex and the corners (W, 0), (0, 0), (W, H), (0, H) at depth ``max(fx, fy) * 1e-3 * size``
    (gui_utils.py:69-86)."""
    W, H, fx, fy, cx, cy = (float(getattr(intr, k)) for k in ("width", "height", "fx", "fy", "cx", "cy"))
    u, v = np.array([W, 0.0, W, 0.0]), np.array([0.0, 0.0, H, H])
    Z = np.ones(4) * max(fx, fy) * 1e-3
    pts = np.vstack([np.zeros(3), np.stack([(u - cx) * Z / fx, (v - cy) * Z / fy, Z], 1)]) * size
    c2w = _np(c2w)
    return pts @ c2w[:3, :3].T + c2w[:3, 3]


_FRUSTUM_LINES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (2, 4), (3, 4))      # gui_utils.py:88


def frustum_segments(c2w, intr, size: float = 1.0) -> np.ndarray:
    """World-space ``[8, 2, 3]``: the eight lines of a camera frustum (gui_utils.py:69-88)."""
    p = frustum_points(c2w, intr, size)
    return np.stack([np.stack([p[i], p[j]]) for i, j in _FRUSTUM_LINES])


def trajectory_segments(centres) -> np.ndarray:
    """World-space ``[n - 1, 2, 3]``: the polyline through ``centres [n, 3]``."""
    c = _np(centres).reshape(-1, 3)
    return np.stack([c[:-1], c[1:]], 1) if c.shape[0] > 1 else np.zeros((0, 2, 3))


def view_behind(cam, intr, size: float = 1.0) -> FreeCamera:
    """The reference's ``view_dir_behind`` (gui_utils.py:28-38): from ``size`` behind the camera towards the centre of its frustum's
    far corners, the image's up direction up."""
    cam = FreeCamera.of(cam)
    p = frustum_points(cam.c2w, intr, size)
    eye = cam.c2w[:3, :3] @ np.array([0.0, 0.0, -1.0]) * size + cam.c2w[:3, 3]
    return look_at(eye, p[1:].mean(0), p[2] - p[4])


def _clip(p, q, lo, hi, axis_fn):
    """Liang-Barsky step: the part of p + t (q - p), t in [lo, hi], with axis_fn(point) >= 0 (axis_fn affine)."""
    a, b = axis_fn(p), axis_fn(q)
    if a < 0.0 and b < 0.0:
        return None
    if a < 0.0:
        lo = max(lo, a / (a - b))
    elif b < 0.0:
        hi = min(hi, a / (a - b))
    return (lo, hi) if lo <= hi else None


def project_segments(segments, cam: FreeCamera, intr) -> np.ndarray:
    """World-space segments ``[N, 2, 3]`` -> ``int32 [N, 5]`` rows ``{x0, y0, x1, y1, source index}`` in 1/16 pixel, for the camera
    ``render()`` uses: clipped against z >= NEAR in float64, projected with the rasteriser's NDC-to-pixel rule
    ``((ndc + 1) S - 1) / 2``, clipped to the image grown by GUARD pixels, rounded half up.  A segment wholly behind the near
    plane or wholly outside the guard rectangle is dropped."""
    segments = _np(segments).reshape(-1, 2, 3)
    W, H, fx, fy, cx, cy = (float(getattr(intr, k)) for k in ("width", "height", "fx", "fy", "cx", "cy"))
    out = []
    for k, (p, q) in enumerate(segments):
        p, q = cam.R @ p + cam.T, cam.R @ q + cam.T
        t = _clip(p, q, 0.0, 1.0, lambda v: v[2] - NEAR)
        if t is None:
            continue
        p, q = (p if t[0] == 0.0 else p + t[0] * (q - p)), (q if t[1] == 1.0 else p + t[1] * (q - p))     # (an unclipped end stays exact)

        def pix(v):
            ndc_x, ndc_y = (2.0 * fx / W) * v[0] / v[2] + (2.0 * cx - W) / W, (2.0 * fy / H) * v[1] / v[2] + (2.0 * cy - H) / H
            return np.array([((ndc_x + 1.0) * W - 1.0) * 0.5, ((ndc_y + 1.0) * H - 1.0) * 0.5])

        a, b = pix(p), pix(q)
        t = (0.0, 1.0)
        for fn in (lambda v: v[0] + GUARD, lambda v: W + GUARD - v[0], lambda v: v[1] + GUARD, lambda v: H + GUARD - v[1]):
            t = _clip(a, b, t[0], t[1], fn)
            if t is None:
                break
        if t is None:
            continue
        a, b = (a if t[0] == 0.0 else a + t[0] * (b - a)), (b if t[1] == 1.0 else a + t[1] * (b - a))
        out.append([math.floor(a[0] * SUBPIXEL + 0.5), math.floor(a[1] * SUBPIXEL + 0.5), math.floor(b[0] * SUBPIXEL + 0.5),
                    math.floor(b[1] * SUBPIXEL + 0.5), k])
    return np.array(out, dtype=np.int32).reshape(-1, 5)


# ---- the map as the viewer takes it ---------------------------------------------------------------------------------------
class Snapshot(NamedTuple):
    """A detached copy of the activated map (viewer/viewer_packet.py:32-59) and of the cameras to draw."""
    means: torch.Tensor
    rotations: torch.Tensor
    scales: torch.Tensor
    opacity: torch.Tensor
    features: torch.Tensor
    obj_idx: Optional[torch.Tensor]         # [P] int64, when the map has an object layer
    keyframes: tuple                        # FreeCamera each
    current: Optional[FreeCamera]
    gt: Optional[FreeCamera]

    @classmethod
    def from_map(cls, gmap, keyframes: Sequence = (), current=None, gt=None) -> "Snapshot":
        with torch.no_grad():
            c = lambda t: t.detach().clone()  # noqa: E731
            obj = object_labels(gmap).clone() if getattr(gmap, "nr_objects", None) is not None else None
            if gt is not None and not isinstance(gt, (FreeCamera, tuple, list)):
                gt = (gt.R_gt, gt.T_gt)
            return cls(c(gmap.get_xyz), c(gmap.get_rotation), c(gmap.get_scaling), c(gmap.get_opacity), c(gmap.get_features), obj,
                       tuple(FreeCamera.of(k) for k in keyframes), None if current is None else FreeCamera.of(current),
                       None if gt is None else FreeCamera.of(gt))

    def overlay_segments(self, intr, cameras=True, trajectory=True, size: float = 1.0):
        """World-space segments ``[N, 2, 3]`` and their colours ``uint8 [N, 3]``, in drawing order (later ones win)."""
        segs, cols = [], []

        def add(s, colour):
            segs.append(s)
            cols.extend([colour] * len(s))

        if trajectory:
            add(trajectory_segments([k.c2w[:3, 3] for k in self.keyframes]), COLOR_TRAJECTORY)
        if cameras:
            for k in self.keyframes:
                add(frustum_segments(k.c2w, intr, size), COLOR_KEYFRAME)
            if self.gt is not None:
                add(frustum_segments(self.gt.c2w, intr, size), COLOR_GT)
            if self.current is not None:
                add(frustum_segments(self.current.c2w, intr, size), COLOR_CURRENT)
        if not segs:
            return np.zeros((0, 2, 3)), np.zeros((0, 3), dtype=np.uint8)
        return np.concatenate(segs), np.array(cols, dtype=np.uint8).reshape(-1, 3)


class _Overlay(NamedTuple):
    segments: Optional[torch.Tensor]        # int32 [S, 4] on the device
    colors: Optional[torch.Tensor]          # uint8 [S, 3]
    S: int


def _check_image(name, t, shape, dtype):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor; the viewer has no CPU path")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {dtype} {tuple(shape)} (got {t.dtype} {tuple(t.shape)})")
    return t.contiguous()


def rasterize_lines(segments: torch.Tensor, scratch: torch.Tensor, W: int, H: int) -> None:
    """``mgs_viewer_lines``: clear the owner image in ``scratch`` and draw ``segments`` (int32 ``[S, 4]``, 1/16 pixel) into it."""
    S = int(segments.shape[0])
    if S:
        segments = _check_image("segments", segments, (S, 4), torch.int32)
    with _device_guard(scratch.device):
        _lib.check(_lib.load().mgs_viewer_lines(W, H, segments.data_ptr() if S else None, S, scratch.data_ptr(), _stream()),
                   "mgs_viewer_lines")


def compose(mode: str, src: torch.Tensor, lut: Optional[torch.Tensor] = None, seg_rgb: Optional[torch.Tensor] = None,
            scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mgs_viewer_compose``: ``uint8 [H, W, 3]`` from ``src`` (``[3, H, W]`` for rgb / segmentation / elipsoids, ``[H, W]`` for
    depth / time); ``seg_rgb`` (uint8 ``[S, 3]``): resolve the owner image ``rasterize_lines`` left in ``scratch`` on top."""
    if mode not in MODES:
        raise ValueError(f"unknown viewer mode {mode!r}: one of {MODES}")
    if not torch.is_tensor(src) or not src.is_cuda:
        raise RuntimeError("src must be a CUDA/HIP tensor; the viewer has no CPU path")
    planar = mode in ("depth", "time")
    if src.dtype != torch.float32 or src.dim() != (2 if planar else 3) or (not planar and src.shape[0] != 3):
        raise ValueError(f"mode {mode!r} takes a float32 {'[H, W]' if planar else '[3, H, W]'} image (got {src.dtype} {tuple(src.shape)})")
    if planar and lut is None:
        raise ValueError("depth and time need the colour table (jet_lut())")
    H, W = int(src.shape[-2]), int(src.shape[-1])
    S = 0 if seg_rgb is None else int(seg_rgb.shape[0])
    if (S or mode == "depth") and scratch is None:
        raise ValueError("depth, and an overlay, need the viewer scratch")
    src = src.contiguous()
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=src.device)
    with _device_guard(src.device):
        _lib.check(_lib.load().mgs_viewer_compose(_COMPOSE_MODE[mode], W, H, src.data_ptr(), _ptr(lut), _ptr(seg_rgb) if S else None,
                                                  S, _ptr(scratch), out.data_ptr(), _stream()), "mgs_viewer_compose")
    return out


def ellipsoids(color: torch.Tensor, threshold: float = ELLIPSOID_THRESHOLD, want_hit: bool = True):
    """``mgs_viewer_ellipsoids`` through the scratch of the differentiable rasteriser forward that produced ``color`` (found as
    ``render_features`` finds them): ``float32 [3, H, W]`` and, with ``want_hit``, the pick buffer ``int32 [H, W]``."""
    t = forward_scratch(color, "ellipsoids")
    out = torch.empty(3, t.H, t.W, dtype=torch.float32, device=t.device)
    hit = torch.empty(t.H, t.W, dtype=torch.int32, device=t.device) if want_hit else None
    with _device_guard(t.device):
        _lib.check(_lib.load().mgs_viewer_ellipsoids(C.byref(t.cam), t.P, t.num_rendered, *t.pointers(), float(threshold),
                                                     out.data_ptr(), _ptr(hit), _stream()), "mgs_viewer_ellipsoids")
    return (out, hit) if want_hit else out


class HeadlessViewer:
    """``frame(snapshot, camera, mode)`` -> ``uint8 [H, W, 3]`` on the device.  ``palette``: ``[K, 3]`` float colours in 0..1 for the
    segmentation mode (the reference draws them at random, slam_viewer.py:88-103; here a fixed generator does)."""

    def __init__(self, intr, background, palette=None):
        self.intr, self.bg = intr, background
        self.W, self.H = int(intr.width), int(intr.height)
        self.palette = palette
        self._lut = self._scratch = None
        self._overlay_key, self._overlay = None, None

    def _device_state(self, dev):
        if self._lut is None:
            self._lut = torch.from_numpy(jet_lut()).to(dev)
            self._scratch = torch.empty(_lib.load().mgs_viewer_scratch_bytes(self.W, self.H) + 256, dtype=torch.uint8, device=dev)
            off = (-self._scratch.data_ptr()) % 256
            self._scratch = self._scratch[off:off + _lib.load().mgs_viewer_scratch_bytes(self.W, self.H)]

    def overlay(self, snapshot: Snapshot, camera: FreeCamera, cameras=True, trajectory=True) -> _Overlay:
        """The projected, clipped and quantised segments of ``snapshot`` for ``camera``, on the device (remembered for the pair)."""
        key = (id(snapshot), id(camera), bool(cameras), bool(trajectory))
        if self._overlay_key != key:
            world, cols = snapshot.overlay_segments(self.intr, cameras, trajectory)
            q = project_segments(world, camera, self.intr)
            dev = snapshot.means.device
            if len(q):
                ov = _Overlay(torch.from_numpy(np.ascontiguousarray(q[:, :4])).to(dev),
                              torch.from_numpy(np.ascontiguousarray(cols[q[:, 4]])).to(dev), len(q))
            else:
                ov = _Overlay(None, None, 0)
            self._overlay_key, self._overlay, self._overlay_refs = key, ov, (snapshot, camera)
        return self._overlay

    def frame(self, snapshot: Snapshot, camera, mode: str = "rgb", scale_modifier: float = 1.0, cameras=True, trajectory=True,
              want_hit: bool = False):
        if mode not in MODES:
            raise ValueError(f"unknown viewer mode {mode!r}: one of {MODES}")
        if mode == "segmentation" and snapshot.obj_idx is None:
            raise ValueError("the segmentation mode needs a map with an object layer (GaussianMap(..., nr_objects=K))")
        if want_hit and mode != "elipsoids":
            raise ValueError("the hit image comes from the ellipsoid walk: want_hit needs mode='elipsoids'")
        if not snapshot.means.is_cuda:
            raise RuntimeError("the snapshot must live on a CUDA/HIP device; the viewer has no CPU path")
        camera = FreeCamera.of(camera)
        dev = snapshot.means.device
        self._device_state(dev)
        ov = self.overlay(snapshot, camera, cameras, trajectory) if (cameras or trajectory) else _Overlay(None, None, 0)
        colors = snapshot.features
        if mode == "segmentation":
            if self.palette is None:
                g = torch.Generator().manual_seed(0)
                self.palette = torch.rand(256, 3, generator=g)
            self.palette = self.palette.to(dev, torch.float32)
            colors = self.palette[snapshot.obj_idx]
        rs = raster_settings(self.intr, self.bg, *camera.tensors(self.intr), scale_modifier=float(scale_modifier))
        P = int(snapshot.means.shape[0])
        args = dict(means3D=snapshot.means, means2D=torch.zeros_like(snapshot.means), opacities=snapshot.opacity,
                    scales=snapshot.scales, rotations=snapshot.rotations)
        hit = None
        if mode == "elipsoids" and P > 0:
            with torch.enable_grad():           # (a forward that keeps its tables: they are what the walk reads)
                color = GaussianRasterizer(rs)(colors_precomp=colors.detach().requires_grad_(True), **args)[0]
            src, hit = ellipsoids(color, ELLIPSOID_THRESHOLD, want_hit=True)
        elif mode == "elipsoids":
            src = torch.zeros(3, self.H, self.W, device=dev)
            hit = torch.full((self.H, self.W), -1, dtype=torch.int32, device=dev)
        else:
            with torch.no_grad():
                color, _, depth, opacity, _ = GaussianRasterizer(rs)(colors_precomp=colors, **args)
            src = depth[0] if mode == "depth" else opacity[0] if mode == "time" else color
        if ov.S:
            rasterize_lines(ov.segments, self._scratch, self.W, self.H)
        img = compose(mode, src, self._lut, ov.colors if ov.S else None, self._scratch)
        return (img, hit) if want_hit else img


def save_png(img: torch.Tensor, path: str) -> None:
    """Write a ``uint8 [H, W, 3]`` frame (synchronises: the one read-back of a frame, and only when it is saved)."""
    from PIL import Image
    Image.fromarray(img.detach().cpu().numpy()).save(path)
