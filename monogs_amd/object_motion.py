"""Rigid object motion: one world-frame SE(3) pose per dynamic object of the map's object layer ("Object motion";
csrc/object_motion.hip).

The reference's configs split a scene's segment ids into ``static``, ``dynamic`` and ``masked`` objects and its map carries a row of
object probabilities per Gaussian, but nothing in it moves a Gaussian.  Here the Gaussians whose label (``labels_of``) is one of
up to 16 dynamic ids are moved by that object's pose, ``x' = R x + t`` and ``q' = quat(R) (x) q``, in one launch, and the gradient of
whatever is rendered from the result is reduced to one se(3) tangent per object, without float atomics, in two.

* ``ObjectPoses``: the poses, the label -> slot table, the deltas and the Adam state; ``step_and_retract`` steps every object in one
  ``mgs_pose_step_batch`` launch and retracts as the camera is retracted, ``T <- exp([rho; theta]^) T``;
* ``transform_objects``: the autograd function around ``mgs_object_transform_forward`` / ``_backward``;
* ``ObjectTracker``: the tracker's loop with the camera fixed and the objects free;
* ``track_dynamic_sequence``: camera and objects over a sequence, frame by frame.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence

import torch

from . import _lib
from . import camera as cam
from . import fused_losses
from .gaussian_map import object_labels
from ._launch import _device_guard, _f32, _ptr, _stream
from .rasterizer import GaussianRasterizer
from .renderer import raster_settings

MAX_MOVING_OBJECTS = _lib.H.MGS_MAX_MOVING_OBJECTS


def _check_ids(ids) -> List[int]:
    ids = [int(i) for i in ids]
    if len(ids) > MAX_MOVING_OBJECTS:
        raise ValueError(f"at most {MAX_MOVING_OBJECTS} moving objects (got {len(ids)})")
    for i in ids:
        if not 0 <= i <= 255:
            raise ValueError(f"object id {i} outside 0..255 (ids are 8-bit)")
    if len(set(ids)) != len(ids):
        raise ValueError(f"duplicate object ids in {ids}")
    return ids


class ObjectPoses:
    """The world-frame poses ``(R [M,3,3], T [M,3])`` of the objects ``dynamic_ids``, identity at start: a Gaussian of object m at
    ``x`` in the map stands at ``R[m] x + T[m]``.  ``slot_of_label`` is the device table (int32 [256]) from an id to its row, -1 for
    every other id.  ``rot_delta`` / ``trans_delta`` ([M,3] parameters, zero between steps) receive the gradients of
    ``transform_objects``; ``step_and_retract`` is the camera's ``PoseAdam.step_and_retract`` for all objects in one launch
    (``mgs_pose_step_batch`` with no exposure and no camera to refresh).

    The learning rates default to the tracker's 0.003 (rotation) and 0.001 (translation).  This is a CHOICE: the reference has no
    object poses and therefore no rates for them; an object in front of a fixed camera is the camera's problem seen from the other
    side, so the camera's rates are the natural start."""

    def __init__(self, dynamic_ids: Sequence[int], device, lr_rot: float = 0.003, lr_trans: float = 0.001, betas=(0.9, 0.999),
                 eps: float = 1e-8):
        self.ids = _check_ids(dynamic_ids)
        self.device = torch.device(device)
        M = self.M = len(self.ids)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.R = torch.eye(3, **f32).repeat(M, 1, 1).contiguous()
        self.T = torch.zeros(M, 3, **f32)
        table = torch.full((256,), -1, dtype=torch.int32)
        for m, i in enumerate(self.ids):
            table[i] = m
        self.slot_of_label = table.to(self.device)
        self.rot_delta = torch.nn.Parameter(torch.zeros(M, 3, **f32))
        self.trans_delta = torch.nn.Parameter(torch.zeros(M, 3, **f32))
        self.lrs, self.betas, self.eps = (float(lr_rot), float(lr_trans)), betas, float(eps)
        self.m, self.v = torch.zeros(M, 8, **f32), torch.zeros(M, 8, **f32)       # the pose step's layout: rot, trans, (a, b unused)
        self.out = torch.zeros(M, 2, **f32)                                        # per object {converged, |tau|}
        self.t_dev = torch.zeros(M, dtype=torch.int32, device=self.device)         # Adam step counts, on the device

    def slot(self, obj_id: int) -> int:
        try:
            return self.ids.index(int(obj_id))
        except ValueError:
            raise KeyError(f"object {obj_id} is not one of the moving objects {self.ids}") from None

    def pose(self, obj_id: int):
        """``(R [3,3], t [3])`` of one object (clones)."""
        m = self.slot(obj_id)
        return self.R[m].clone(), self.T[m].clone()

    @torch.no_grad()
    def set_pose(self, obj_id: int, R, t):
        m = self.slot(obj_id)
        self.R[m].copy_(torch.as_tensor(R, dtype=torch.float32))
        self.T[m].copy_(torch.as_tensor(t, dtype=torch.float32))

    @torch.no_grad()
    def reset_optimizer(self):
        """Fresh Adam state without re-allocating (what ``PoseAdam.reset`` is to the camera): captured graphs keep pointing at it."""
        self.m.zero_(); self.v.zero_(); self.out.zero_(); self.t_dev.zero_()
        self.rot_delta.zero_(); self.trans_delta.zero_()

    def zero_grad(self):
        self.rot_delta.grad = None
        self.trans_delta.grad = None

    @staticmethod
    def _row_ptrs(g, M):
        """Device address of each object's three gradient floats (``g``: [M,3] with unit stride along the row, or None)."""
        if g is None:
            return [None] * M
        if g.stride(1) != 1:
            g = g.contiguous()
        return [g.data_ptr() + 4 * m * g.stride(0) for m in range(M)]

    @torch.no_grad()
    def step_and_retract(self, converged_threshold: float = 1e-4) -> torch.Tensor:
        """One Adam step on every object's deltas and the retraction, in ONE launch; the deltas are zero again afterwards.  Returns
        the device tensor ``out [M,2]``, ``{converged (0/1), |tau|}`` per object; nothing is read back."""
        M = self.M
        if M == 0:
            return self.out
        lib = _lib.load()
        g_rot, g_trans = self._row_ptrs(self.rot_delta.grad, M), self._row_ptrs(self.trans_delta.grad, M)
        flat = []
        for m in range(M):
            flat += [self.R[m].data_ptr(), self.T[m].data_ptr(), self.rot_delta[m].data_ptr(), self.trans_delta[m].data_ptr(), None, None,
                     g_rot[m], g_trans[m], None, None, self.m[m].data_ptr(), self.v[m].data_ptr(), self.t_dev[m:m + 1].data_ptr(),
                     self.out[m].data_ptr(), None, None, None, None]
        arr = (C.c_void_p * len(flat))(*flat)
        with _device_guard(self.device):
            _lib.check(lib.mgs_pose_step_batch(M, arr, self.lrs[0], self.lrs[1], 0.0, self.betas[0], self.betas[1], self.eps,
                                               float(converged_threshold), 0, _stream()), "mgs_pose_step_batch")
        return self.out


class _TransformObjects(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, rot, rot_delta, trans_delta, labels, poses):
        lib = _lib.load()
        x = _f32(xyz.detach(), "xyz")
        q = None if rot is None else _f32(rot.detach(), "rot")
        P = int(x.shape[0])
        if labels.dtype != torch.uint8 or tuple(labels.shape) != (P,) or labels.device != x.device or not labels.is_contiguous():
            raise ValueError(f"labels must be a contiguous uint8 [{P}] tensor on {x.device} (labels_of(gmap))")
        if x.dim() != 2 or x.shape[1] != 3 or (q is not None and tuple(q.shape) != (P, 4)):
            raise ValueError("xyz must be [P,3] and rot [P,4]")
        x_out = torch.empty_like(x)
        q_out = None if q is None else torch.empty_like(q)
        with _device_guard(x.device):
            _lib.check(lib.mgs_object_transform_forward(P, poses.M, _ptr(labels), poses.slot_of_label.data_ptr(), _ptr(poses.R),
                                                        _ptr(poses.T), _ptr(x), _ptr(q), _ptr(x_out), _ptr(q_out), _stream()),
                       "mgs_object_transform_forward")
        ctx.poses, ctx.P, ctx.has_rot = poses, P, q is not None
        # R as it is NOW: the retraction that follows the backward of a later iteration must not reach this one
        ctx.save_for_backward(labels, x_out, q_out if q_out is not None else torch.empty(0, device=x.device), poses.R.clone())
        ctx.set_materialize_grads(False)      # an unused output's gradient arrives as None, not as a zero fill
        return x_out, q_out

    @staticmethod
    def backward(ctx, g_x, g_q):
        lib = _lib.load()
        labels, x_out, q_out, R = ctx.saved_tensors
        poses, P = ctx.poses, ctx.P
        dev = x_out.device
        need = ctx.needs_input_grad           # xyz, rot, rot_delta, trans_delta
        f32 = dict(dtype=torch.float32, device=dev)
        with _device_guard(dev):
            g_x = torch.zeros(P, 3, **f32) if g_x is None else _f32(g_x, "grad_xyz")
            g_q = None if (g_q is None or not ctx.has_rot) else _f32(g_q, "grad_rot")
            d_x = torch.empty(P, 3, **f32) if need[0] else None
            d_q = torch.empty(P, 4, **f32) if (need[1] and g_q is not None) else None
            d_tau = torch.empty(poses.M, 6, **f32)
            scratch = torch.empty(lib.mgs_object_motion_scratch_bytes(P, poses.M), dtype=torch.uint8, device=dev)
            _lib.check(lib.mgs_object_transform_backward(P, poses.M, _ptr(labels), poses.slot_of_label.data_ptr(), _ptr(R), _ptr(x_out),
                                                         _ptr(q_out) if g_q is not None else None, _ptr(g_x), _ptr(g_q), _ptr(d_x),
                                                         _ptr(d_q), _ptr(d_tau), scratch.data_ptr(), _stream()),
                       "mgs_object_transform_backward")
        # (views of the [M,6] result, rho then theta: autograd takes them as .grad without a copy kernel)
        return d_x, d_q, d_tau[:, 3:] if need[2] else None, d_tau[:, :3] if need[3] else None, None, None


def transform_objects(xyz: torch.Tensor, rot, labels_u8: torch.Tensor, poses: ObjectPoses):
    """``(xyz', rot')``: the Gaussians of the moving objects at their poses, every other one copied bit for bit; ``rot`` (and then
    ``rot'``) may be None.  ``labels_u8``: ``labels_of(gmap)``.  The backward leaves one se(3) tangent per object in
    ``poses.rot_delta.grad`` (theta) and ``poses.trans_delta.grad`` (rho) -- the deltas are zero at evaluation, the pose is retracted
    as the camera's is -- and hands ``xyz`` / ``rot`` their gradients when they ask for them.  No host synchronisation."""
    if not isinstance(poses, ObjectPoses):
        raise TypeError("poses must be an ObjectPoses")
    return _TransformObjects.apply(xyz, rot, poses.rot_delta, poses.trans_delta, labels_u8, poses)


def labels_of(gmap) -> torch.Tensor:
    """``object_labels(gmap)`` as the contiguous uint8 [P] the kernels read."""
    return object_labels(gmap).to(torch.uint8).contiguous()


class ObjectTracker:
    """Tracks the objects of ``poses`` in a frame whose camera pose is known: the tracker's iteration (``tracking.track_eager``) with
    the camera fixed, the map detached and the object poses free.  An iteration is ``transform_objects`` -> rasteriser ->
    ``fused_losses.get_loss_tracking`` -> backward -> ``poses.step_and_retract``; the loss looks at the pixels whose segmentation
    id is dynamic, its depth zero elsewhere (``frames.mask_objects(vp, ids, keep=True, border=border)``).  The loop ends when every
    object's step is below 1e-4, as the camera tracker's does; that flag is the only read-back of an iteration.

    ``border = 2`` pixels of the object's silhouette are left out, a CHOICE with a measured reason ("Object motion"): the
    tracking loss counts only pixels the render covers with opacity above 0.99, and behind an object that has moved since it was mapped
    the map is empty, so with the silhouette included the loss is lowest 22 mm away from the true pose on the dynamic room; with a border
    of 1 to 3 pixels it is lowest within 1.3 mm of it."""

    def __init__(self, intr, gmap, bg, poses: ObjectPoses, border: int = 2):
        self.intr, self.bg, self.poses, self.border = intr, bg, poses, int(border)
        with torch.no_grad():
            self.map = tuple(t.detach().contiguous() for t in (gmap.get_xyz, gmap.get_rotation, gmap.get_scaling, gmap.get_opacity,
                                                               gmap.get_features))
            self.labels = labels_of(gmap)
        self.zero2d = torch.zeros_like(self.map[0])
        dev = self.map[0].device
        self.cam3 = (torch.empty(4, 4, device=dev), torch.empty(4, 4, device=dev), torch.empty(3, device=dev))
        self.target = None

    @torch.no_grad()
    def load(self, vp):
        """The frame to track in: its pose is the camera, its dynamic pixels the target.  Fresh optimiser state."""
        from .frames import mask_objects
        self.target = mask_objects(vp, self.poses.ids, keep=True, border=self.border)
        for p in (self.target.exposure_a, self.target.exposure_b):      # the frame's exposure is the camera's business: fixed here
            p.requires_grad_(False)
        cam.fused_camera_matrices(self.target.R, self.target.T, self.intr.projection_matrix, out=self.cam3)
        self.poses.reset_optimizer()

    def iteration(self) -> torch.Tensor:
        """One iteration on the loaded frame; returns ``poses.out`` (device).  No host synchronisation of its own: capturable after
        one eager iteration (the rasteriser's capacity hint)."""
        xyz, rot, sca, opa, col = self.map
        xyz2, rot2 = transform_objects(xyz, rot, self.labels, self.poses)
        color, _, depth, opacity, _ = GaussianRasterizer(raster_settings(self.intr, self.bg, *self.cam3))(
            means3D=xyz2, means2D=self.zero2d, opacities=opa, colors_precomp=col, scales=sca, rotations=rot2)
        self.poses.zero_grad()
        fused_losses.get_loss_tracking(color, depth, opacity, self.target).backward()
        return self.poses.step_and_retract()

    def track(self, vp, max_iters: int) -> int:
        """Tracks the objects in ``vp`` from the poses they hold; returns the iterations run."""
        self.load(vp)
        n_it = 0
        for _ in range(max_iters):
            out = self.iteration()
            n_it += 1
            if self.poses.M == 0 or bool(out[:, 0].min().item() > 0.5):
                break
        return n_it


class MovedMap:
    """What ``render_map`` reads of a map, with the moving objects at their current poses (detached: tracking takes no map gradient)."""
    fused_adam = False

    def __init__(self, gmap, labels, poses):
        with torch.no_grad():
            self.get_xyz, self.get_rotation = transform_objects(gmap.get_xyz.detach(), gmap.get_rotation.detach(), labels, poses)
            self.get_scaling, self.get_opacity, self.get_features = (gmap.get_scaling.detach(), gmap.get_opacity.detach(),
                                                                     gmap.get_features.detach())


def track_dynamic_sequence(frames, intr, gmap, bg, dynamic_ids: Sequence[int], camera: str = "gt", max_iters: int = 100,
                           border: int = 2) -> Dict:
    """Frame 0 anchors the run (the map was built from it: its camera is its ground truth, the objects stand at the identity); every
    later frame first gets its camera -- ``camera="gt"``: the ground-truth pose; ``"track"``: ``track_eager`` from the previous
    frame's estimate on ``mask_objects(vp, ids, border=border)``, against the map with the objects at their last pose -- and then its
    objects, ``ObjectTracker.track`` from the poses of the previous frame (``border``: ``ObjectTracker``'s).  Returns ``camera`` (a list of ``(R, t)`` per frame), ``objects``
    (``{id: [(R, t) per frame]}``, world frame, relative to frame 0) and ``iters`` (a list of ``(frame, camera iterations, object
    iterations)`` for the frames after the first; 0 camera iterations with ``"gt"``)."""
    from .frames import Viewpoint, mask_objects
    from .tracking import track_eager
    if camera not in ("gt", "track"):
        raise ValueError('camera must be "gt" or "track"')
    dev = gmap.get_xyz.device
    poses = ObjectPoses(dynamic_ids, dev)
    tracker = ObjectTracker(intr, gmap, bg, poses, border=border)
    cams = [(frames[0].R_gt.clone(), frames[0].T_gt.clone())]
    objs = {i: [poses.pose(i)] for i in poses.ids}
    iters = []
    for f in frames[1:]:
        n_cam = 0
        if camera == "gt":
            R, t = f.R_gt.clone(), f.T_gt.clone()
        else:
            vc = mask_objects(f, poses.ids, border=border)
            vc.update_RT(cams[-1][0].clone(), cams[-1][1].clone())
            n_cam = track_eager(vc, intr, MovedMap(gmap, tracker.labels, poses), bg, max_iters)
            R, t = vc.R.detach().clone(), vc.T.detach().clone()
        vo = Viewpoint(f.frame_idx, f.rgb, f.depth, dev, gt_R=f.R_gt, gt_T=f.T_gt, mask=f.mask, grad_mask=f.grad_mask,
                       segmentation=f.segmentation)
        vo.update_RT(R, t)
        n_obj = tracker.track(vo, max_iters)
        cams.append((R, t))
        for i in poses.ids:
            objs[i].append(poses.pose(i))
        iters.append((int(f.frame_idx), n_cam, n_obj))
    return dict(camera=cams, objects=objs, iters=iters)


def object_position_error(pose, gt_pose, centre) -> float:
    """Distance (metres) between where ``pose = (R, t)`` and where ``gt_pose`` put the point ``centre`` of the object's frame-0
    placement: the object's counterpart of ``frames.position_error``."""
    c = torch.as_tensor(centre, dtype=torch.float64)
    at = lambda p: torch.as_tensor(p[0]).detach().cpu().double() @ c + torch.as_tensor(p[1]).detach().cpu().double()  # noqa: E731
    return float((at(pose) - at(gt_pose)).norm())
