"""Geometry out of the map: TSDF fusion of depth images into a dense voxel grid and an indexed triangle mesh from it
(``csrc/tsdf.hip``; the specification is DESIGN.md, "TSDF fusion and mesh extraction").  No counterpart in the reference.

``TSDFVolume.integrate`` is one launch with no host synchronisation (capturable in a hipGraph); ``extract`` is five launches, ONE
read-back of two counts, two more launches.  ``fuse_map`` renders the map from a list of viewpoints and integrates what the
rasteriser returns (its un-normalised depth, its opacity, its colour).  ``mesh_stats`` is plain torch on the device: evaluation,
not a hot path."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from .camera import cached_camera_tensors, fused_camera_matrices
from ._launch import _device_guard, _f32, _stream


class TriangleMesh(NamedTuple):
    vertices: torch.Tensor               # [V,3] float32
    triangles: torch.Tensor              # [T,3] int32
    colors: Optional[torch.Tensor]       # [V,3] float32 in 0..1, or None


class TSDFVolume:
    """A dense grid of ``dims = (nx, ny, nz)`` voxels of edge ``voxel``; ``origin`` (world metres) is the centre of voxel (0,0,0).
    Planes ``tsdf`` (1), ``weight`` (0) and, with ``color``, ``r g b`` (0), each [nz, ny, nx] float32."""

    def __init__(self, origin, voxel: float, dims, device, color: bool = True, trunc: Optional[float] = None, max_weight: float = 64):
        self.origin = tuple(float(x) for x in (origin.tolist() if torch.is_tensor(origin) else origin))
        self.voxel, self.dims = float(voxel), tuple(int(d) for d in dims)
        self.device = torch.device(device)
        self.trunc = 4.0 * self.voxel if trunc is None else float(trunc)
        self.max_weight, self.color = float(max_weight), bool(color)
        nx, ny, nz = self.dims
        if min(self.dims) <= 0 or nx * ny * nz >= 1 << 31:
            raise ValueError(f"dims {self.dims}: every dimension positive and nx ny nz below 2^31")
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume lives on the GPU; there is no CPU path")
        self._planes = torch.empty(5 if color else 2, nz, ny, nx, dtype=torch.float32, device=self.device)
        self.reset()
        v = self._vol = _lib.MgsTsdfVolume()
        v.nx, v.ny, v.nz = nx, ny, nz
        v.origin = (C.c_float * 3)(*self.origin)
        v.voxel = self.voxel
        ptr = [self._planes[i].data_ptr() for i in range(self._planes.shape[0])] + [None] * 3
        v.tsdf, v.weight, v.r, v.g, v.b = ptr[:5]
        self.stats = dict(integrations=0, readbacks=0)

    @classmethod
    def for_bounds(cls, lo, hi, voxel: float, device, **kw):
        """The smallest grid whose voxel centres cover the box ``lo .. hi`` (origin = ``lo``)."""
        lo = [float(x) for x in (lo.tolist() if torch.is_tensor(lo) else lo)]
        hi = [float(x) for x in (hi.tolist() if torch.is_tensor(hi) else hi)]
        import math
        dims = [int(math.ceil((h - l) / voxel - 1e-6)) + 1 for l, h in zip(lo, hi)]
        return cls(lo, voxel, dims, device, **kw)

    def reset(self):
        self._planes.zero_()
        self._planes[0].fill_(1.0)

    def planes(self):
        """``(tsdf, weight, r, g, b)`` as views ([nz, ny, nx]); ``r g b`` are None for a volume without colour."""
        p = self._planes
        return (p[0], p[1]) + ((p[2], p[3], p[4]) if self.color else (None, None, None))

    def integrate(self, depth, R, T=None, intr=None, rgb=None, opacity=None, depth_min=0.01, depth_max=0.0, opacity_min=0.9,
                  cull=True):
        """Fuse one frame.  ``R``, ``T``: world->camera device tensors, or ``R`` a viewpoint (``.R``, ``.T``) and ``T`` None.
        ``depth`` [H,W] (or [1,H,W]); with ``opacity`` it is the rasteriser's un-normalised depth.  ``cull=False``: test use."""
        lib = _lib.load()
        if intr is None:
            raise ValueError("integrate needs the intrinsics")
        if T is None and hasattr(R, "R") and hasattr(R, "T"):
            view = cached_camera_tensors(R, R.R, R.T, intr.projection_matrix)[0]
        else:
            view = fused_camera_matrices(R, T, intr.projection_matrix)[0]
        H, W = int(intr.height), int(intr.width)
        depth = _f32(depth.detach(), "depth")
        if depth.numel() != H * W:
            raise ValueError(f"depth has {tuple(depth.shape)}, the intrinsics say {H} x {W}")
        fr = _lib.MgsTsdfFrame()
        fr.width, fr.height, fr.depth, fr.viewmatrix = W, H, depth.data_ptr(), view.data_ptr()
        keep = [depth, view]
        if opacity is not None:
            opacity = _f32(opacity.detach(), "opacity")
            if opacity.numel() != H * W:
                raise ValueError("opacity must have the depth's size")
            fr.opacity = opacity.data_ptr()
            keep.append(opacity)
        if rgb is not None and self.color:
            rgb = _f32(rgb.detach(), "rgb")
            if tuple(rgb.shape) != (3, H, W):
                raise ValueError(f"rgb must be [3,{H},{W}]")
            fr.rgb = rgb.data_ptr()
            keep.append(rgb)
        fr.fx, fr.fy, fr.cx, fr.cy = float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy)
        fr.trunc, fr.depth_min, fr.depth_max = self.trunc, float(depth_min), float(depth_max)
        fr.opacity_min, fr.max_weight, fr.flags = float(opacity_min), self.max_weight, 0 if cull else 1
        with _device_guard(self.device):
            _lib.check(lib.mgs_tsdf_integrate(C.byref(self._vol), C.byref(fr), _stream()), "mgs_tsdf_integrate")
        self.stats["integrations"] += 1

    def extract(self, min_weight: float = 1) -> TriangleMesh:
        lib = _lib.load()
        dev = self.device
        nx, ny, nz = self.dims
        scratch = torch.empty(lib.mgs_tsdf_extract_scratch_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        with _device_guard(dev):
            _lib.check(lib.mgs_tsdf_extract_count(C.byref(self._vol), float(min_weight), scratch.data_ptr(), counts.data_ptr(),
                                                  _stream()), "mgs_tsdf_extract_count")
            V, T = (int(c) & 0xFFFFFFFF for c in counts.cpu().tolist())            # the ONE read-back
            self.stats["readbacks"] += 1
            if V >= 1 << 31 or T >= 1 << 31:
                raise RuntimeError(f"the mesh has {V} vertices / {T} triangles: beyond 32-bit indices")
            vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
            colors = torch.empty(V, 3, dtype=torch.float32, device=dev) if self.color else None
            triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
            _lib.check(lib.mgs_tsdf_extract_emit(C.byref(self._vol), scratch.data_ptr(), vertices.data_ptr() if V else None,
                                                 colors.data_ptr() if (colors is not None and V) else None,
                                                 triangles.data_ptr() if T else None, V, T, _stream()), "mgs_tsdf_extract_emit")
        return TriangleMesh(vertices, triangles, colors)


@torch.no_grad()
def fuse_map(gmap, viewpoints, intr, bg, volume: TSDFVolume, timing: bool = False, depth: str = "mean", max_std: float = 0.0,
             **integrate_kw):
    """One no-grad ``render()`` of the map per viewpoint (detached activations, as ``evaluation.eval_rendering``), each integrated into
    ``volume`` with the render's ``depth`` / ``opacity`` / ``render``.  Nothing is read back.  ``{renders, integrations, readbacks}``;
    ``timing``: also ``integrate_ms``, the device time of the integrations alone (events around each; one synchronisation at the end).
    ``depth="median"``: the render keeps its tables and the frame's depth is ``surface.surface_depth``'s median, gated by
    ``opacity_min`` (``integrate``'s default where not given) and, with ``max_std > 0``, by the depth's spread along the ray; it is
    integrated without an opacity plane, the gates having zeroed the pixels ``integrate`` must skip."""
    from .gaussian_optim import activate
    from .renderer import render
    if depth not in ("mean", "median"):
        raise ValueError(f"depth must be \"mean\" or \"median\", got {depth!r}")
    if depth == "mean" and max_std:
        raise ValueError("max_std gates the median depth: it needs depth=\"median\"")
    stats = dict(renders=0, integrations=0, readbacks=0)
    events = []
    if not len(gmap):
        return dict(stats, integrate_ms=0.0) if timing else stats
    rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
    xyz, feat = gmap._xyz.detach(), gmap._rgb.detach()
    for vp in viewpoints:
        if depth == "median":
            from .surface import render_with_tables, surface_depth
            pkg = render_with_tables(vp, intr, (xyz, rot, scales3, opac, feat), bg)
            median = surface_depth(pkg["render"], want=("median", "variance") if max_std > 0 else ("median",),
                                   min_opacity=integrate_kw.get("opacity_min", 0.9), max_std=max_std).median
        else:
            pkg = render(vp, intr, xyz, rot, scales3, opac, feat, bg)
        stats["renders"] += 1
        if timing:
            events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            events[-1][0].record()
        if depth == "median":
            volume.integrate(median, vp, None, intr, rgb=pkg["render"], opacity=None, **integrate_kw)
        else:
            volume.integrate(pkg["depth"], vp, None, intr, rgb=pkg["render"], opacity=pkg["opacity"], **integrate_kw)
        if timing:
            events[-1][1].record()
        stats["integrations"] += 1
    if timing:
        torch.cuda.synchronize(volume.device)
        stats["integrate_ms"] = float(sum(a.elapsed_time(b) for a, b in events))
    return stats


def mesh_from_map(gmap, viewpoints, intr, bg, voxel: float, path: Optional[str] = None, max_voxels: int = 1 << 29,
                  depth: str = "mean", max_std: float = 0.0) -> dict:
    """What ``run_slam(mesh_path=...)`` does at the end of a run: a volume over the bounds of the map's centres (padded by the
    truncation distance), ``fuse_map`` over ``viewpoints``, ``extract``, and the PLY at ``path``.  Returns ``{path, vertices, triangles,
    voxel, integrate_ms, extract_ms, mesh}``.  The bounds are read back (six floats): this runs once, after the run.  ``depth``,
    ``max_std``: as ``fuse_map``."""
    import time
    from .ply_io import save_mesh_ply
    if not len(gmap):
        raise ValueError("the map is empty: nothing to fuse")
    xyz = gmap._xyz.detach()
    pad = 4.0 * float(voxel)
    lo, hi = (xyz.min(dim=0).values - pad).tolist(), (xyz.max(dim=0).values + pad).tolist()
    n = 1
    for l, h in zip(lo, hi):
        n *= int((h - l) / voxel) + 2
    if n > max_voxels:
        raise ValueError(f"a {voxel} m grid over the map's bounds {lo} .. {hi} has {n} voxels (limit {max_voxels}): choose a larger voxel")
    vol = TSDFVolume.for_bounds(lo, hi, float(voxel), xyz.device)
    stats = fuse_map(gmap, viewpoints, intr, bg, vol, timing=True, depth=depth, max_std=max_std)
    torch.cuda.synchronize(xyz.device)
    t0 = time.perf_counter()
    mesh = vol.extract()
    torch.cuda.synchronize(xyz.device)
    extract_ms = 1e3 * (time.perf_counter() - t0)
    if path is not None:
        save_mesh_ply(path, mesh)
    return dict(path=None if path is None else str(path), vertices=int(mesh.vertices.shape[0]), triangles=int(mesh.triangles.shape[0]),
                voxel=float(voxel), integrate_ms=stats["integrate_ms"], extract_ms=extract_ms, mesh=mesh)


@torch.no_grad()
def mesh_stats(mesh: TriangleMesh) -> dict:
    """Area, signed volume (positive for outward normals of a closed surface), and the number of undirected edges used by exactly one
    triangle (``boundary_edges``) or by more than two (``non_manifold_edges``), from the device tensors."""
    v, t = mesh.vertices.double(), mesh.triangles.long()
    if t.shape[0] == 0:
        return dict(vertices=int(v.shape[0]), triangles=0, area=0.0, volume=0.0, boundary_edges=0, non_manifold_edges=0)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = torch.cross(b - a, c - a, dim=1)
    e = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = e.min(dim=1).values * int(v.shape[0]) + e.max(dim=1).values
    _, cnt = torch.unique(key, return_counts=True)
    return dict(vertices=int(v.shape[0]), triangles=int(t.shape[0]), area=float(0.5 * n.norm(dim=1).sum()),
                volume=float((a * n).sum() / 6.0), boundary_edges=int((cnt == 1).sum()), non_manifold_edges=int((cnt > 2).sum()))
