"""A triangle mesh seen from a camera: depth, triangle id, vertex colour and face label images of an indexed mesh
(``csrc/mesh_render.hip``; the specification is DESIGN.md, "Mesh rendering"), and Depth L1, the 2-D figure of the Replica
reconstruction tables, between two meshes rendered from the same views.  No counterpart in the reference, which has no mesh.

``MeshRenderer.render`` is six launches with no host synchronisation and no read-back (capturable in a hipGraph); the image is
bitwise reproducible and does not depend on the order of the triangles.  ``eval_depth_l1`` launches everything and reads back ONE
table."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from .camera import cached_camera_tensors, fused_camera_matrices
from ._launch import _device_guard, _f32, _stream

MESH_ONE_SIDED, MESH_NO_SMALL = 1, 2
WANTS = ("depth", "tri_id", "rgb", "label")


def _cuda(t, what: str, dtype) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA/HIP tensor; there is no CPU path")
    return t.detach().to(dtype).contiguous()


class MeshRenderer:
    """Owns the scratch and the output images of one image size (``intr``) on ``device``.  The tensors ``render`` returns are the
    renderer's own buffers: the next call overwrites them (clone what must outlive it)."""

    def __init__(self, intr, device):
        self.intr, self.device = intr, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MeshRenderer lives on the GPU; there is no CPU path")
        H, W = int(intr.height), int(intr.width)
        self.H, self.W = H, W
        dev = self.device
        self._out = dict(depth=torch.zeros(H, W, dtype=torch.float32, device=dev), tri_id=torch.full((H, W), -1, dtype=torch.int32, device=dev),
                         rgb=torch.zeros(3, H, W, dtype=torch.float32, device=dev), label=torch.full((H, W), -1, dtype=torch.int32, device=dev))
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._cam = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in ((4, 4), (4, 4), (3,)))
        self._scratch, self._scratch_T = None, -1
        self.stats = dict(renders=0, readbacks=0)

    def _scratch_for(self, T: int) -> torch.Tensor:
        if T > self._scratch_T:
            n = _lib.load().mgs_mesh_render_scratch_bytes(T, self.W, self.H)
            self._scratch, self._scratch_T = torch.empty(n, dtype=torch.uint8, device=self.device), T
        return self._scratch

    def render(self, mesh, R, T=None, want: Sequence[str] = ("depth",), face_labels: Optional[torch.Tensor] = None, bg=None,
               near: float = 0.01, far: float = 0.0, two_sided: bool = True, fuse_small: bool = True) -> dict:
        """``mesh`` (``.vertices`` [V,3], ``.triangles`` [T,3], ``.colors`` [V,3] or None) from the world->camera pose ``R``, ``T``
        (device tensors), or ``R`` a viewpoint (``.R``, ``.T``) and ``T`` None.  ``want``: any of ``depth`` [H,W] float32 (always
        written; 0: nothing hit), ``tri_id`` [H,W] int32 (-1), ``rgb`` [3,H,W] float32 (``bg``, default black) and ``label`` [H,W]
        int32 (``face_labels[tri_id]``; -1).  ``two_sided=False``: only triangles whose geometric normal faces the camera.
        ``fuse_small=False`` (test and measurement use): no triangle is rasterised by the setup kernel; the image is bit-identical."""
        lib = _lib.load()
        want = tuple(want)
        for w in want:
            if w not in WANTS:
                raise ValueError(f"want must hold names from {WANTS}, got {w!r}")
        v = _cuda(mesh.vertices, "mesh.vertices", torch.float32)
        t = _cuda(mesh.triangles, "mesh.triangles", torch.int32)
        if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3:
            raise RuntimeError(f"mesh.vertices must be [V,3] and mesh.triangles [T,3], got {tuple(v.shape)} and {tuple(t.shape)}")
        keep = [v, t]
        p = _lib.MgsMeshRender()
        p.V, p.T = v.shape[0], t.shape[0]
        p.vertices, p.triangles = v.data_ptr() if p.V else None, t.data_ptr() if p.T else None
        if "rgb" in want:
            if mesh.colors is None:
                raise ValueError("rgb wanted from a mesh without colours")
            c = _cuda(mesh.colors, "mesh.colors", torch.float32)
            if tuple(c.shape) != tuple(v.shape):
                raise ValueError(f"mesh.colors must be [{p.V},3]")
            p.colors = c.data_ptr() if p.V else 0x100          # (never read: no triangle is set up without a vertex)
            p.rgb = self._out["rgb"].data_ptr()
            keep.append(c)
        if "label" in want:
            if face_labels is None:
                raise ValueError("label wanted without face_labels")
            fl = _cuda(face_labels, "face_labels", torch.int32)
            if tuple(fl.shape) != (p.T,):
                raise ValueError(f"face_labels must be [{p.T}], got {tuple(fl.shape)}")
            p.face_labels = fl.data_ptr() if p.T else 0x100
            p.label = self._out["label"].data_ptr()
            keep.append(fl)
        if "tri_id" in want:
            p.tri_id = self._out["tri_id"].data_ptr()
        with _device_guard(self.device):
            if T is None and hasattr(R, "R") and hasattr(R, "T"):
                view = cached_camera_tensors(R, R.R, R.T, self.intr.projection_matrix)[0]
            else:
                view = fused_camera_matrices(_cuda(R, "R", torch.float32), _cuda(T, "T", torch.float32), self.intr.projection_matrix,
                                             out=self._cam)[0]
            intr = self.intr
            p.viewmatrix, p.W, p.H = view.data_ptr(), self.W, self.H
            p.fx, p.fy, p.cx, p.cy = float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy)
            p.near, p.far = float(near), float(far)
            p.flags = (0 if two_sided else MESH_ONE_SIDED) | (0 if fuse_small else MESH_NO_SMALL)
            p.bg = (C.c_float * 3)(*([0.0, 0.0, 0.0] if bg is None else [float(x) for x in (bg.tolist() if torch.is_tensor(bg) else bg)]))
            p.depth, p.status = self._out["depth"].data_ptr(), self._status.data_ptr()
            scratch = self._scratch_for(p.T)
            _lib.check(lib.mgs_mesh_render(C.byref(p), scratch.data_ptr(), _stream()), "mgs_mesh_render")
        self.stats["renders"] += 1
        return {k: self._out[k] for k in dict.fromkeys(("depth",) + want)}

    def status_word(self) -> torch.Tensor:
        """The device status word [1] int32 (bit 0: some triangle named a vertex outside [0, V)); nothing is read back."""
        return self._status

    def status(self) -> int:
        """Reads the status word back, clears it, and raises on bit 0."""
        st = int(self._status.cpu().item())
        self.stats["readbacks"] += 1
        self._status.zero_()
        if st & 1:
            raise Exception("mgs_mesh_render: a triangle names a vertex outside [0, V)")
        return st


def render_mesh(mesh, R, T, intr, **kw) -> dict:
    """The one-shot form of ``MeshRenderer.render`` (checks the status word: one read-back)."""
    r = MeshRenderer(intr, mesh.vertices.device if torch.is_tensor(mesh.vertices) and mesh.vertices.is_cuda else "cpu")
    out = r.render(mesh, R, T, **kw)
    r.status()
    return out


def depth_l1_row(a: torch.Tensor, b: torch.Tensor, max_depth: float = 0.0, out: Optional[torch.Tensor] = None, scratch=None) -> torch.Tensor:
    """Device float64 [3]: the sum of ``|a - b|`` over the pixels where both depth images are ``> 0`` (and, with ``max_depth > 0``,
    both ``<= max_depth``), that pixel count, and the count of pixels with ``b > 0``.  Nothing is read back."""
    lib = _lib.load()
    if not (torch.is_tensor(a) and torch.is_tensor(b) and a.is_cuda and b.is_cuda):
        raise RuntimeError("depth images must be CUDA/HIP tensors; there is no CPU path")
    a, b = _f32(a.detach(), "a"), _f32(b.detach(), "b")
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"two [H,W] images of one size, got {tuple(a.shape)} and {tuple(b.shape)}")
    row = torch.empty(3, dtype=torch.float64, device=a.device) if out is None else out
    with _device_guard(a.device):
        if scratch is None:
            scratch = torch.empty(lib.mgs_depth_l1_scratch_bytes(), dtype=torch.uint8, device=a.device)
        _lib.check(lib.mgs_depth_l1(a.shape[1], a.shape[0], a.data_ptr(), b.data_ptr(), float(max_depth), row.data_ptr(),
                                    scratch.data_ptr(), _stream()), "mgs_depth_l1")
    return row


@torch.no_grad()
def eval_depth_l1(rec, gt, viewpoints, intr, max_depth: float = 0.0) -> dict:
    """Depth L1 between a reconstructed and a ground-truth mesh: both are rendered from every view (``viewpoints``: objects with
    ``.R``, ``.T`` or ``(R, T)`` pairs); ``depth_l1_m`` is the mean over the views of the per-view mean of ``|d_rec - d_gt|`` over the
    pixels BOTH meshes hit (views without such a pixel do not count), ``coverage`` the share of ground-truth-hit pixels that the
    reconstruction also hits.  THE PROJECT'S OWN DEFINITION: the published protocols differ in how they treat holes, so parity with
    them is unpinned.  ``readbacks`` is 1: the table of all views with the two status words."""
    viewpoints = list(viewpoints)
    dev = gt.vertices.device
    r_rec, r_gt = MeshRenderer(intr, dev), MeshRenderer(intr, dev)
    n = len(viewpoints)
    table = torch.zeros(n + 1, 3, dtype=torch.float64, device=dev)
    with _device_guard(dev):
        scratch = torch.empty(_lib.load().mgs_depth_l1_scratch_bytes(), dtype=torch.uint8, device=dev)
    for i, vp in enumerate(viewpoints):
        R, T = (vp[0], vp[1]) if isinstance(vp, (tuple, list)) else (vp, None)
        a = r_rec.render(rec, R, T)["depth"]
        b = r_gt.render(gt, R, T)["depth"]
        depth_l1_row(a, b, max_depth, out=table[i], scratch=scratch)
    table[n, 0:1] = r_rec.status_word().to(torch.float64)
    table[n, 1:2] = r_gt.status_word().to(torch.float64)
    rows = table.cpu().tolist()                                        # the ONE read-back
    for st, what in ((rows[n][0], "the reconstruction"), (rows[n][1], "the ground truth")):
        if int(st) & 1:
            raise Exception(f"mgs_mesh_render: {what}: a triangle names a vertex outside [0, V)")
    per_view = [dict(depth_l1_m=s / c if c else float("nan"), pixels=int(c), gt_pixels=int(g)) for s, c, g in rows[:n]]
    means = [p["depth_l1_m"] for p in per_view if p["pixels"]]
    both, in_gt = sum(p["pixels"] for p in per_view), sum(p["gt_pixels"] for p in per_view)
    return dict(depth_l1_m=sum(means) / len(means) if means else float("nan"), coverage=both / in_gt if in_gt else float("nan"),
                views=n, per_view=per_view, max_depth_m=float(max_depth), readbacks=1)
