"""Synthetic RGB-D sequences with ground-truth poses, for the measurements whose datasets (BASELINE configs 3-4) are not
available offline: an opaque box room ray-cast analytically (``make_room_sequence``: what bench.py runs, survives the
reference's pruning) and, historically, a seeded cloud of Gaussians rendered by the rasteriser itself (``make_sequence``).
A sequence on disk comes from ``monogs_amd.dataset.dataset_frames`` in the same ``(frames, intr)`` form."""
from __future__ import annotations

import math
from typing import List

import torch

from . import camera as cam
from .frames import Intrinsics, Viewpoint
from .gaussian_map import GaussianMap
from .map_step import render_map
from .synthetic import make_scene


def make_sequence(n_frames: int, intrinsics="fr3_office", n_gaussians=60000, seed=11, device="cuda:0"):
    """Ground-truth map + a smooth camera path; frames rendered by the rasteriser itself."""
    sc = make_scene(n_gaussians, intrinsics, seed=seed, near_fraction=0.0, mean_radius_px=9.0, device=device)
    intr = Intrinsics(sc.intr, device)
    gt = GaussianMap(device)
    gt._xyz, gt._rgb = sc.means3D, sc.colors
    gt._opacity = torch.logit(sc.opacities.clamp(0.05, 0.95) * 0 + 0.9)     # mostly opaque surface-like splats
    gt._scaling, gt._rotation = torch.log(sc.scales), sc.rotations
    bg = torch.zeros(3, device=device)
    T0 = torch.eye(4, device=device)
    T0[:3, :3], T0[:3, 3] = sc.R, sc.t
    frames: List[Viewpoint] = []
    with torch.no_grad():
        for i in range(n_frames):
            d = cam.se3_exp(torch.tensor([0.004 * i, -0.002 * i, 0.001 * i, 0.0, 0.0015 * i, 0.0005 * i], device=device))
            Tm = d @ T0
            vp = Viewpoint(i, torch.zeros(3, intr.height, intr.width, device=device),
                           torch.ones(intr.height, intr.width, device=device), device)
            vp.update_RT(Tm[:3, :3], Tm[:3, 3])
            pkg = render_map(vp, intr, gt, bg)
            depth = torch.where(pkg["opacity"][0] > 0.5, pkg["depth"][0] / pkg["opacity"][0].clamp_min(1e-6),
                                torch.zeros_like(pkg["depth"][0]))
            frames.append(Viewpoint(i, pkg["render"].clamp(0, 1), depth, device, gt_R=Tm[:3, :3], gt_T=Tm[:3, 3]))
    return frames, intr


# ---- an OPAQUE-surface stand-in: a box room with furniture, ray-cast analytically -----------------------------------------
# The cloud of `make_sequence` is semi-transparent by construction (its "depth" is a blend over several layers), so a map
# fitted to it never gets past the reference's 0.7 opacity pruning threshold.  A real sequence shows opaque surfaces: this
# one is a 6 x 3 x 6 m room with four boxes standing in it, every pixel's colour and z-depth computed in closed form
# (ray / axis-aligned-box intersection, a procedural texture of the hit point), seen from a hand-held-like camera path.
_ROOM_HALF = (3.0, 1.5, 3.0)
_ROOM_BOXES = (   # (lo, hi) in world metres; y points down in the first camera, the floor is y = +1.5
    ((-2.4, 0.55, 1.1), (-0.9, 1.5, 2.3)),      # a desk
    ((0.9, -0.3, 1.8), (1.9, 1.5, 2.8)),        # a cabinet
    ((-0.5, 0.9, 0.9), (0.4, 1.5, 1.6)),        # a crate in front
    ((2.2, 0.2, -0.5), (3.0, 1.5, 0.9)),        # a shelf on the right wall
)


def _room_texture(p, axis, sid):
    """Colour of the surface point ``p`` [N,3] whose normal is along ``axis`` [N]; ``sid`` [N] picks the base colour."""
    dev = p.device
    ia = torch.where(axis == 0, 1, 0)
    ib = torch.where(axis == 2, 1, 2)
    a = torch.gather(p, 1, ia[:, None])[:, 0]
    b = torch.gather(p, 1, ib[:, None])[:, 0]
    base = torch.tensor([[0.78, 0.72, 0.62], [0.55, 0.66, 0.80], [0.70, 0.80, 0.62], [0.82, 0.60, 0.58], [0.60, 0.60, 0.72],
                         [0.85, 0.80, 0.55], [0.50, 0.72, 0.70], [0.75, 0.55, 0.75], [0.62, 0.78, 0.85], [0.80, 0.68, 0.50]],
                        device=dev)[sid % 10]
    two_pi = 2.0 * math.pi
    ph = sid.to(torch.float32) * 1.7
    slow = 0.5 + 0.5 * torch.sin(two_pi * 0.45 * a + ph) * torch.sin(two_pi * 0.38 * b + 0.6 * ph)
    # a soft checker (edges 3 cm wide) and a fine weave: image gradients everywhere, as a textured office has
    chk = torch.tanh(torch.sin(two_pi * a / 0.8) * torch.sin(two_pi * b / 0.8) * 12.0)
    fine = torch.sin(two_pi * a / 0.11 + ph) * torch.sin(two_pi * b / 0.13)
    lum = 0.62 + 0.16 * slow + 0.14 * chk + 0.06 * fine
    tint = torch.stack([torch.sin(two_pi * 0.21 * a + ph), torch.sin(two_pi * 0.17 * b + 2.0 + ph),
                        torch.sin(two_pi * 0.13 * (a + b) + 4.0)], 1) * 0.08
    return (base * lum[:, None] + tint).clamp(0.02, 0.98)


ROOM_SURFACES = 6 + 3 * len(_ROOM_BOXES)       # surface ids raycast_room can return: six walls, three face axes per box


@torch.no_grad()
def raycast_room(R, t, k, device, with_ids=False):
    """(rgb [3,H,W], depth [H,W]) of the room seen by the world->camera pose (R, t); ``with_ids``: also the id [H,W] (int32,
    below ``ROOM_SURFACES``) of the surface every ray hit.  Pixel (x, y) looks along
    ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1): the rasteriser's pixel convention (``px = fx X/Z + cx - 0.5``) and the
    back-projection's (/root/reference/gaussian_splatting/scene/gaussian_model.py:232-236)."""
    H, W = k["H"], k["W"]
    ys, xs = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float32),
                            torch.arange(W, device=device, dtype=torch.float32), indexing="ij")
    dc = torch.stack([(xs + 0.5 - k["cx"]) / k["fx"], (ys + 0.5 - k["cy"]) / k["fy"], torch.ones_like(xs)], -1).reshape(-1, 3)
    R, t = R.to(device), t.to(device)
    o = -(R.t() @ t)
    d = dc @ R                                            # R^T d, row form
    d = torch.where(d.abs() < 1e-9, torch.full_like(d, 1e-9), d)
    half = torch.tensor(_ROOM_HALF, device=device)
    t_wall = (torch.where(d > 0, half, -half) - o) / d    # the room from inside: the nearest exit plane
    best, axis = t_wall.min(dim=1)
    sid = axis * 2 + (torch.gather(d, 1, axis[:, None])[:, 0] > 0).long()
    for bi, (lo, hi) in enumerate(_ROOM_BOXES):
        lo, hi = torch.tensor(lo, device=device), torch.tensor(hi, device=device)
        t1, t2 = (lo - o) / d, (hi - o) / d
        tn, ax = torch.minimum(t1, t2).max(dim=1)
        tf = torch.maximum(t1, t2).min(dim=1).values
        hit = (tn < tf) & (tn > 1e-3) & (tn < best)
        best = torch.where(hit, tn, best)
        axis = torch.where(hit, ax, axis)
        sid = torch.where(hit, 6 + bi * 3 + ax, sid)
    p = o + best[:, None] * d
    rgb = _room_texture(p, axis, sid)
    if with_ids:
        return rgb.t().reshape(3, H, W).contiguous(), best.reshape(H, W).contiguous(), sid.to(torch.int32).reshape(H, W).contiguous()
    return rgb.t().reshape(3, H, W).contiguous(), best.reshape(H, W).contiguous()


def room_surface_distance(points: torch.Tensor) -> torch.Tensor:
    """Unsigned distance [N] of ``points`` [N,3] (world metres) to the room's surfaces: the union of its six walls and the faces of
    the four boxes, in closed form (distance to the boundary of an axis-aligned box: outside ``|max(q, 0)|``, inside ``-max(q)``
    with ``q = |p - centre| - half``).  Plain torch; for evaluating a reconstructed mesh, nothing on a hot path."""
    p = points.to(torch.float64)
    boxes = [((-_ROOM_HALF[0], -_ROOM_HALF[1], -_ROOM_HALF[2]), _ROOM_HALF)] + list(_ROOM_BOXES)
    best = None
    for lo, hi in boxes:
        lo, hi = torch.tensor(lo, dtype=p.dtype, device=p.device), torch.tensor(hi, dtype=p.dtype, device=p.device)
        q = (p - 0.5 * (lo + hi)).abs() - 0.5 * (hi - lo)
        out = q.clamp_min(0.0).norm(dim=1)
        d = torch.where(out > 0, out, -q.max(dim=1).values)
        best = d if best is None else torch.minimum(best, d)
    return best.to(points.dtype)


def room_rectangles(boxes=None):
    """The room's true surfaces as axis-aligned rectangles ``(axis, side, (a, a_lo, a_hi), (b, b_lo, b_hi))``: the plane ``x[axis] =
    side`` over ``[a_lo, a_hi] x [b_lo, b_hi]`` of the other two axes -- the six walls and the six faces of every box, from the tables
    ``room_surface_distance`` uses (a box standing on the floor or against a wall keeps that face: it is part of the union's distance).
    ``boxes``: the ``(lo, hi)`` boxes to take the faces of instead."""
    out = []
    for lo, hi in ([((-_ROOM_HALF[0], -_ROOM_HALF[1], -_ROOM_HALF[2]), _ROOM_HALF)] + list(_ROOM_BOXES)) if boxes is None else boxes:
        for ax in range(3):
            a, b = [i for i in range(3) if i != ax]
            for side in (lo[ax], hi[ax]):
                out.append((ax, float(side), (a, float(lo[a]), float(hi[a])), (b, float(lo[b]), float(hi[b]))))
    return out


def _room_grids(max_edge: float, boxes=None):
    """``room_rectangles`` with the dicing of ``room_mesh``: ``(rectangle number, axis, side, (a, a_lo, a_hi), (b, b_lo, b_hi), na, nb)``."""
    cell = float(max_edge) / math.sqrt(2.0)
    for n, (ax, side, (a, a_lo, a_hi), (b, b_lo, b_hi)) in enumerate(room_rectangles(boxes)):
        na, nb = max(1, int(math.ceil((a_hi - a_lo) / cell - 1e-9))), max(1, int(math.ceil((b_hi - b_lo) / cell - 1e-9)))
        yield n, ax, side, (a, a_lo, a_hi), (b, b_lo, b_hi), na, nb


def _rectangle_surface_id(n: int, ax: int) -> int:
    """The id ``raycast_room(with_ids=True)`` reports for rectangle ``n`` of ``room_rectangles``: walls ``2 axis + (the + side)``,
    the faces of box ``k`` ``6 + 3 k + axis``."""
    return 2 * ax + (n % 2) if n < 6 else 6 + 3 * ((n - 6) // 6) + ax


def room_mesh(device, max_edge: float = 0.1, dtype=torch.float32, colors: bool = False):
    """The room's true surfaces (``room_rectangles``) as a ``TriangleMesh``, every rectangle diced into a grid of cells
    split along one diagonal so that no edge -- the diagonals included -- exceeds ``max_edge``: the visibility cull of
    ``mesh_eval.seen_vertices`` is per vertex.  Vertices are computed in float64 and stored as ``dtype``.  ``colors``: the room's
    texture (``raycast_room``'s) evaluated at the vertices; without, the mesh has no colours."""
    return _grid_mesh(_room_grids(max_edge), device, dtype, _rectangle_surface_id if colors else None)


def _grid_mesh(grids, device, dtype, surface_id):
    """The diced rectangles ``grids`` (``_room_grids``) as one ``TriangleMesh``; ``surface_id(n, axis)``: the texture id of rectangle
    ``n`` for ``_room_texture`` at the vertices, or None: no colours."""
    import numpy as np
    from .tsdf import TriangleMesh
    colors = surface_id is not None
    verts, tris, cols, base = [], [], [], 0
    for n, ax, side, (a, a_lo, a_hi), (b, b_lo, b_hi), na, nb in grids:
        A, B = np.meshgrid(np.linspace(a_lo, a_hi, na + 1), np.linspace(b_lo, b_hi, nb + 1), indexing="ij")
        p = np.zeros(A.shape + (3,))
        p[..., a], p[..., b], p[..., ax] = A, B, side
        verts.append(p.reshape(-1, 3))
        if colors:
            pt = torch.from_numpy(verts[-1]).to(torch.float32)
            cols.append(_room_texture(pt, torch.full((len(pt),), ax, dtype=torch.long),
                                      torch.full((len(pt),), surface_id(n, ax), dtype=torch.long)))
        i, j = np.meshgrid(np.arange(na), np.arange(nb), indexing="ij")
        v00 = (base + i * (nb + 1) + j).reshape(-1)
        v10, v01, v11 = v00 + (nb + 1), v00 + 1, v00 + (nb + 1) + 1
        tris.append(np.stack([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)], 1).reshape(-1, 3))
        base += (na + 1) * (nb + 1)
    v = torch.from_numpy(np.concatenate(verts)).to(dtype).to(device)
    t = torch.from_numpy(np.concatenate(tris).astype(np.int32)).to(device)
    return TriangleMesh(v, t, torch.cat(cols).to(torch.float32).to(device) if colors else None)


def room_mesh_surface_ids(max_edge: float = 0.1) -> torch.Tensor:
    """[T] int32 (CPU): per triangle of ``room_mesh(max_edge=max_edge)``, the surface id ``raycast_room(with_ids=True)`` reports for it."""
    out = []
    for n, ax, _, _, _, na, nb in _room_grids(max_edge):
        out.append(torch.full((2 * na * nb,), _rectangle_surface_id(n, ax), dtype=torch.int32))
    return torch.cat(out)


@torch.no_grad()
def make_mesh_sequence(mesh, poses, intrinsics, device, face_labels=None, bg=(0.0, 0.0, 0.0)):
    """``(frames, intr)`` in the shape of ``make_room_sequence``: one ``Viewpoint`` per world->camera pose ``(R, t)`` of ``poses`` with the
    coloured mesh rendered on the device (``mesh_render.MeshRenderer``) as ``rgb`` and ``depth``, the pose as ground truth and, with
    ``face_labels`` [T], the label image as ``segmentation``.  A mesh without colours is refused.  ``mesh`` may be a function of the
    frame number (a scene that changes; the triangle count, hence ``face_labels``, stays)."""
    mesh_of = mesh if callable(mesh) else (lambda i: mesh)
    if mesh_of(0).colors is None:
        raise ValueError("make_mesh_sequence needs a mesh with vertex colours")
    from .mesh_render import MeshRenderer
    k = dict(cam.INTRINSICS[intrinsics]) if isinstance(intrinsics, str) else dict(intrinsics)
    intr = Intrinsics(k, device)
    renderer = MeshRenderer(intr, device)
    want = ("depth", "rgb") + (("label",) if face_labels is not None else ())
    frames: List[Viewpoint] = []
    for i, (R, t) in enumerate(poses):
        R = torch.as_tensor(R, dtype=torch.float32).to(device).contiguous()
        t = torch.as_tensor(t, dtype=torch.float32).to(device).contiguous()
        out = renderer.render(mesh_of(i), R, t, want=want, face_labels=face_labels, bg=bg)
        frames.append(Viewpoint(i, out["rgb"].clone(), out["depth"].clone(), device, gt_R=R, gt_T=t,
                                segmentation=out["label"].clone() if face_labels is not None else None))
    renderer.status()
    return frames, intr


def room_path_pose(s: float):
    """The world->camera pose ``(R, t)`` (CPU float32) at parameter ``s`` of the hand-held-like path of ``make_room_sequence``."""
    c = torch.tensor([0.35 * math.sin(0.022 * s) - 0.2, 0.05 * math.sin(0.05 * s) + 0.1, -1.6 + 0.25 * (1 - math.cos(0.02 * s))])
    yaw, pitch = 0.0055 * s - 0.1, 0.05 + 0.03 * math.sin(0.04 * s)
    Rwc = cam.so3_exp(torch.tensor([0.0, yaw, 0.0])) @ cam.so3_exp(torch.tensor([pitch, 0.0, 0.0]))   # camera -> world
    Rcw = Rwc.t().contiguous()
    return Rcw, -(Rcw @ c)


def make_room_sequence(n_frames: int, intrinsics="fr3_office", device="cuda:0", step_scale: float = 1.0,
                       with_segmentation: bool = False):
    """``n_frames`` RGB-D frames of the room along a smooth hand-held-like path (about 1 cm and 0.3 degrees per frame at
    ``step_scale`` 1: the inter-frame motion of a 30 Hz TUM sequence), ground-truth poses attached.  ``with_segmentation``:
    every frame also carries ``segmentation``, the id of the surface each pixel's ray hit (``raycast_room``)."""
    k = dict(cam.INTRINSICS[intrinsics]) if isinstance(intrinsics, str) else dict(intrinsics)
    intr = Intrinsics(k, device)
    frames: List[Viewpoint] = []
    for i in range(n_frames):
        Rcw, tcw = room_path_pose(step_scale * i)
        rgb, depth, *seg = raycast_room(Rcw, tcw, k, device, with_ids=with_segmentation)
        frames.append(Viewpoint(i, rgb, depth, device, gt_R=Rcw.to(device), gt_T=tcw.to(device),
                                segmentation=seg[0] if seg else None))
    return frames, intr


# ---- a dynamic scene: the room with one more box, which moves ------------------------------------------------------------------
DYNAMIC_BOX = ((-0.30, -0.45, 0.50), (0.35, 0.25, 1.10))      # (lo, hi) at frame 0: in the middle of the first view, 2.4 m away
DYNAMIC_BOX_ID = ROOM_SURFACES                                # its segmentation id: the first one the room does not use


def dynamic_box_motion(i: int):
    """The default ``object_motion`` of ``make_dynamic_room_sequence``: the world-frame ``(R, t)`` (CPU float32) of the box at frame
    ``i`` relative to frame 0 -- its centre moves 1.02 cm per frame along (0.8, -0.2, 0.6) cm while it turns 0.5 degrees per frame
    about the axis (0.2, 1, 0.1) through that centre."""
    lo, hi = (torch.tensor(v, dtype=torch.float64) for v in DYNAMIC_BOX)
    c0 = 0.5 * (lo + hi)
    axis = torch.tensor([0.2, 1.0, 0.1], dtype=torch.float64)
    R = cam.so3_exp(axis / axis.norm() * math.radians(0.5) * i)
    c = c0 + i * torch.tensor([0.008, -0.002, 0.006], dtype=torch.float64)
    return R.to(torch.float32), (c - R @ c0).to(torch.float32)


@torch.no_grad()
def make_dynamic_room_sequence(n_frames: int, intrinsics, device="cuda:0", object_motion=None, step_scale: float = 1.0):
    """``(frames, intr, object_poses)``: the room (``room_mesh(colors=True)``, faces labelled with the ids of ``raycast_room``) plus one
    box, ``DYNAMIC_BOX`` diced to 2 cm edges, textured like the room's surfaces and labelled ``DYNAMIC_BOX_ID``, which is moved by
    ``object_motion(i) -> (R, t)`` (world frame, relative to frame 0; default ``dynamic_box_motion``, about 1 cm and 0.5 degrees per
    frame; ``lambda i: (eye, zeros)`` holds it still) and rendered through ``make_mesh_sequence`` from the camera path of
    ``make_room_sequence``.  Every frame carries ``segmentation``; ``object_poses[i]`` is the ground-truth ``(R, t)`` of the box at frame
    ``i`` (device float32)."""
    from .tsdf import TriangleMesh
    motion = dynamic_box_motion if object_motion is None else object_motion
    room = room_mesh(device, colors=True)
    box = _grid_mesh(_room_grids(0.02, boxes=[DYNAMIC_BOX]), device, torch.float32, lambda n, ax: 6 + ax)      # the desk's three base colours
    tris = torch.cat((room.triangles, box.triangles + room.vertices.shape[0]))
    cols = torch.cat((room.colors, box.colors))
    labels = torch.cat((room_mesh_surface_ids().to(device), torch.full((box.triangles.shape[0],), DYNAMIC_BOX_ID, dtype=torch.int32,
                                                                       device=device)))
    object_poses = [tuple(torch.as_tensor(x, dtype=torch.float32).to(device).contiguous() for x in motion(i)) for i in range(n_frames)]

    def mesh_of(i):
        R, t = object_poses[i]
        return TriangleMesh(torch.cat((room.vertices, box.vertices @ R.t() + t)), tris, cols)
    poses = [room_path_pose(step_scale * i) for i in range(n_frames)]
    frames, intr = make_mesh_sequence(mesh_of, poses, intrinsics, device, face_labels=labels)
    return frames, intr, object_poses
