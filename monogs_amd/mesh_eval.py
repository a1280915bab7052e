"""How good a reconstructed surface is: accuracy, completion, completion ratio, Chamfer-L1 and precision / recall / F-score between
area-weighted samples of a reconstructed and a ground-truth mesh, both first culled to what the cameras saw (``csrc/mesheval.hip``;
the specification is DESIGN.md, "Reconstruction evaluation").  No counterpart in the reference, which has no mesh.

``nearest_distance`` is the hot path (a cross-set nearest neighbour, exact); ``sample_mesh``, ``seen_vertices`` and the reduction
are the other kernels.  ``eval_reconstruction`` launches all of it and reads back ONE vector."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from .camera import cached_camera_tensors, fused_camera_matrices
from ._launch import _device_guard, _f32, _stream
from .tsdf import TriangleMesh

NN_FORCE_ALL_PAIRS, NN_FORCE_MORTON = 1, 2
_PATHS = {None: 0, "all_pairs": NN_FORCE_ALL_PAIRS, "morton": NN_FORCE_MORTON}


def _points(t: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA/HIP tensor; there is no CPU path")
    t = t.detach().to(torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{what} must be [N,3], got {tuple(t.shape)}")
    return t


def _mesh(mesh, what: str):
    v = _points(mesh.vertices, f"{what}.vertices")
    t = mesh.triangles
    if not t.is_cuda:
        raise RuntimeError(f"{what}.triangles must be a CUDA/HIP tensor; there is no CPU path")
    t = t.detach().to(torch.int32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{what}.triangles must be [T,3], got {tuple(t.shape)}")
    return v, t


def nn_grid_min() -> int:
    """The number of targets from which ``nearest_distance`` takes the Morton-box path (below: the all-pairs sweep)."""
    return int(_lib.load().mgs_nn_grid_min())


def nearest_distance(queries: torch.Tensor, targets: torch.Tensor, want_index: bool = False, path: Optional[str] = None):
    """``d2`` [Q] float32: the squared distance of every query to its nearest target; with ``want_index`` also ``index`` [Q] int32,
    the smallest target index that attains it.  No targets: ``+inf`` and ``-1``.  ``path``: None (by size), ``"all_pairs"`` or
    ``"morton"`` -- both give the same bits."""
    lib = _lib.load()
    q, t = _points(queries, "queries"), _points(targets, "targets")
    if path not in _PATHS:
        raise ValueError(f"path must be one of {list(_PATHS)}")
    Q, P = q.shape[0], t.shape[0]
    d2 = torch.empty(Q, dtype=torch.float32, device=q.device)
    index = torch.empty(Q, dtype=torch.int32, device=q.device) if want_index else None
    with _device_guard(q.device):
        scratch = torch.empty(lib.mgs_nn_scratch_bytes(Q, P), dtype=torch.uint8, device=q.device)
        _lib.check(lib.mgs_nn_dist2(Q, P, q.data_ptr(), t.data_ptr() if P else None, _PATHS[path], d2.data_ptr(),
                                    index.data_ptr() if want_index else None, scratch.data_ptr(), _stream()), "mgs_nn_dist2")
    return (d2, index) if want_index else d2


def _sample_launch(mesh, n: int, seed: int, keep, want_triangles: bool):
    """The launches of ``sample_mesh``: ``(points, tri_index or None, area [1] float64 device, status [1] int32 device)``."""
    lib = _lib.load()
    v, t = _mesh(mesh, "mesh")
    dev = v.device
    V, T, n = v.shape[0], t.shape[0], int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    if V == 0 or T == 0:
        raise Exception("mgs_mesh_sample: the mesh has no kept area")
    if keep is not None:
        if not keep.is_cuda:
            raise RuntimeError("keep must be a CUDA/HIP tensor; there is no CPU path")
        keep = keep.detach().to(torch.uint8).contiguous()
        if tuple(keep.shape) != (T,):
            raise ValueError(f"keep must be [{T}], got {tuple(keep.shape)}")
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev) if want_triangles else None
    area = torch.empty(1, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _device_guard(dev):
        scratch = torch.empty(lib.mgs_mesh_sample_scratch_bytes(T), dtype=torch.uint8, device=dev)
        _lib.check(lib.mgs_mesh_sample(V, T, v.data_ptr(), t.data_ptr(), keep.data_ptr() if keep is not None else None, n,
                                       int(seed) & 0xFFFFFFFF, points.data_ptr() if n else None, tri.data_ptr() if want_triangles else None,
                                       area.data_ptr(), status.data_ptr(), scratch.data_ptr(), _stream()), "mgs_mesh_sample")
    return points, tri, area, status


def _sample_verdict(area: float, status: float, what: str = "mesh"):
    if int(status) & 1:
        raise Exception(f"mgs_mesh_sample: {what}: a triangle names a vertex outside [0, V)")
    if not area > 0.0:
        raise Exception(f"mgs_mesh_sample: {what} has no kept area")


def sample_mesh(mesh, n: int, seed: int = 0, keep: Optional[torch.Tensor] = None, want_triangles: bool = False):
    """``n`` area-weighted, stratified points [n,3] on the triangles of ``mesh`` whose ``keep`` byte is set (None: all); with
    ``want_triangles`` also the triangle [n] int32 of each and the kept area in square metres.  Reads back the area and the status word
    (one copy): an out-of-range vertex index and a mesh without kept area are errors."""
    points, tri, area, status = _sample_launch(mesh, n, seed, keep, want_triangles)
    a, st = torch.cat([area, status.to(torch.float64)]).cpu().tolist()
    _sample_verdict(a, st)
    return (points, tri, a) if want_triangles else points


def _view_of(vp, intr):
    if isinstance(vp, (tuple, list)):
        return fused_camera_matrices(vp[0], vp[1], intr.projection_matrix)[0]
    return cached_camera_tensors(vp, vp.R, vp.T, intr.projection_matrix)[0]


def render_depths(mesh, viewpoints, intr):
    """One depth image [H,W] per view of ``mesh`` rendered from it (``mesh_render.MeshRenderer``): the occlusion test of
    ``depths="render"``.  ``viewpoints`` as in ``seen_vertices``."""
    from .mesh_render import MeshRenderer
    renderer = MeshRenderer(intr, mesh.vertices.device)
    out = []
    for vp in viewpoints:
        R, T = (vp[0], vp[1]) if isinstance(vp, (tuple, list)) else (vp, None)
        out.append(renderer.render(mesh, R, T)["depth"].clone())
    return out


def seen_vertices(mesh, viewpoints, intr, depths=None, depth_min: float = 0.01, depth_max: float = 0.0, occlusion_eps: float = 0.03,
                  occluder=None):
    """bool [V]: the vertices some view sees -- camera-space ``z`` in ``[depth_min, depth_max]`` (``depth_max <= 0``: no far limit), the
    pixel of ``TSDFVolume.integrate`` inside the image and, with ``depths`` (one [H,W] image per view), ``depth > 0`` there and
    ``z <= depth + occlusion_eps``.  ``depths="render"``: the images are the mesh ``occluder`` rendered from every view
    (``render_depths``).  ``viewpoints``: objects with ``.R``, ``.T`` (world->camera) or ``(R, T)`` pairs.  One launch per view."""
    lib = _lib.load()
    v = _points(mesh.vertices, "mesh.vertices")
    dev = v.device
    H, W = int(intr.height), int(intr.width)
    viewpoints = list(viewpoints)
    if isinstance(depths, str):
        if depths != "render":
            raise ValueError(f'depths must be None, a list of images or "render", got {depths!r}')
        if occluder is None:
            raise ValueError('depths="render" needs the mesh to render as occluder=')
        depths = render_depths(occluder, viewpoints, intr)
    if depths is not None and len(depths) != len(viewpoints):
        raise ValueError("depths must hold one image per viewpoint")
    seen = torch.zeros(v.shape[0], dtype=torch.uint8, device=dev)
    with _device_guard(dev):
        for i, vp in enumerate(viewpoints):
            view = _view_of(vp, intr)
            depth = None
            if depths is not None:
                depth = _f32(depths[i].detach(), "depth")
                if depth.numel() != H * W:
                    raise ValueError(f"depth has {tuple(depth.shape)}, the intrinsics say {H} x {W}")
            _lib.check(lib.mgs_mesh_mark_seen(v.shape[0], v.data_ptr(), view.data_ptr(), W, H, float(intr.fx), float(intr.fy),
                                              float(intr.cx), float(intr.cy), depth.data_ptr() if depth is not None else None,
                                              float(depth_min), float(depth_max), float(occlusion_eps), seen.data_ptr(), _stream()),
                       "mgs_mesh_mark_seen")
    return seen.bool()


def cull_mesh(mesh, seen: torch.Tensor) -> TriangleMesh:
    """The triangles with at least one seen vertex, in their order; the vertices stay.  Plain torch indexing: it runs once."""
    t = mesh.triangles
    keep = seen[t.long()].any(dim=1)
    return TriangleMesh(mesh.vertices, t[keep].contiguous(), mesh.colors)


def recon_metrics(d2: torch.Tensor, thresholds) -> torch.Tensor:
    """Device float64 ``[2 + K]``: the sum of ``sqrt(d2)`` over the finite entries, their number, and for each of the ``K <= 8``
    thresholds (metres) the number with ``sqrt(d2)`` below it.  Nothing is read back."""
    lib = _lib.load()
    if not d2.is_cuda:
        raise RuntimeError("d2 must be a CUDA/HIP tensor; there is no CPU path")
    d2 = d2.detach().to(torch.float32).contiguous().reshape(-1)
    thr = [float(x) for x in thresholds]
    if len(thr) > 8:
        raise ValueError("at most eight thresholds")
    out = torch.empty(2 + len(thr), dtype=torch.float64, device=d2.device)
    with _device_guard(d2.device):
        scratch = torch.empty(lib.mgs_recon_metrics_scratch_bytes(), dtype=torch.uint8, device=d2.device)
        _lib.check(lib.mgs_recon_metrics(d2.shape[0], d2.data_ptr() if d2.shape[0] else None, len(thr), (C.c_float * max(len(thr), 1))(*thr),
                                         out.data_ptr(), scratch.data_ptr(), _stream()), "mgs_recon_metrics")
    return out


def figures(acc_sum, acc_n, acc_below, comp_sum, comp_n, comp_below) -> dict:
    """The seven figures from the two directions' sums and counts (plain arithmetic on the read-back vector)."""
    accuracy = acc_sum / acc_n if acc_n else float("nan")
    completion = comp_sum / comp_n if comp_n else float("nan")
    precision = acc_below / acc_n if acc_n else float("nan")
    recall = comp_below / comp_n if comp_n else float("nan")
    fscore = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return dict(accuracy_m=accuracy, completion_m=completion, completion_ratio=recall, chamfer_l1_m=0.5 * (accuracy + completion),
                precision=precision, recall=recall, fscore=fscore)


@torch.no_grad()
def eval_reconstruction(rec, gt, n_samples: int = 200_000, threshold: float = 0.05, seed: int = 0, viewpoints=None, intr=None,
                        depths=None, return_samples: bool = False, **cull_kw) -> dict:
    """Accuracy (mean distance reconstruction -> ground truth), completion (ground truth -> reconstruction), completion ratio (share
    of ground-truth samples within ``threshold``), Chamfer-L1 (the mean of the first two) and precision / recall / F-score at
    ``threshold``, between ``n_samples`` samples of each mesh (seeds ``seed`` and ``seed + 1``).  With ``viewpoints`` (and ``intr``,
    optionally ``depths``) both meshes are first culled: only triangles with a vertex ``seen_vertices`` reports are sampled (``cull_mesh``'s rule);
    ``depths="render"``: the ground-truth mesh rendered from each viewpoint is the occlusion test for both.  ``readbacks`` is 1: the result vector
    (sums, counts, areas, status words).  ``return_samples``: also ``rec_samples``, ``gt_samples``, ``rec_d2``, ``gt_d2`` (device)."""
    keep_rec = keep_gt = None
    if isinstance(depths, str) and depths != "render":
        raise ValueError(f'depths must be None, a list of images or "render", got {depths!r}')
    if viewpoints is not None:
        if intr is None:
            raise ValueError("culling by viewpoints needs the intrinsics")
        viewpoints = list(viewpoints)
        if isinstance(depths, str):
            depths = render_depths(gt, viewpoints, intr)
        # (cull_mesh's rule as the sampler's keep mask: indexing the triangles by it would read their number back)
        keep_rec = seen_vertices(rec, viewpoints, intr, depths, **cull_kw)[rec.triangles.long()].any(dim=1)
        keep_gt = seen_vertices(gt, viewpoints, intr, depths, **cull_kw)[gt.triangles.long()].any(dim=1)
    p_rec, _, a_rec, s_rec = _sample_launch(rec, n_samples, seed, keep_rec, False)
    p_gt, _, a_gt, s_gt = _sample_launch(gt, n_samples, seed + 1, keep_gt, False)
    d_acc = nearest_distance(p_rec, p_gt)
    d_comp = nearest_distance(p_gt, p_rec)
    m_acc, m_comp = recon_metrics(d_acc, [threshold]), recon_metrics(d_comp, [threshold])
    vec = torch.cat([m_acc, m_comp, a_rec, a_gt, s_rec.to(torch.float64), s_gt.to(torch.float64)]).cpu().tolist()     # the ONE read-back
    _sample_verdict(vec[6], vec[8], "the reconstruction" + (" (culled)" if viewpoints is not None else ""))
    _sample_verdict(vec[7], vec[9], "the ground truth" + (" (culled)" if viewpoints is not None else ""))
    out = figures(vec[0], vec[1], vec[2], vec[3], vec[4], vec[5])
    out.update(rec_area_m2=vec[6], gt_area_m2=vec[7], n_samples=int(n_samples), threshold_m=float(threshold), readbacks=1)
    if return_samples:
        out.update(rec_samples=p_rec, gt_samples=p_gt, rec_d2=d_acc, gt_d2=d_comp)
    return out
