"""Rigid object motion on the GPU ("Object motion"): ``mgs_object_transform_forward`` / ``_backward`` against the
float64 mirror (tests/object_motion_mirror.py), ``transform_objects`` through the rasteriser against plain torch, one captured
``ObjectTracker`` iteration against eager ones, and the box of ``make_dynamic_room_sequence`` tracked with the ground-truth and with
the tracked camera.

Bounds (u = 2^-24, one float32 rounding of a number below 1 in magnitude, relative):
  * a moved mean: three fused multiply-adds, each rounding once, one unit of margin: 4 u (|x|_1 + |t|_inf) per component (|R| <= 1);
  * a moved quaternion (|q| = 1): 8 u;  a static row: bit-equal;
  * each of the [M,6] sums: (n_m + 2) u sum|term| -- any summation order of n_m terms, plus the cross product's roundings --
    with sum|term| the absolute values of the products that enter the sum, from the mirror;  an empty slot: exactly 0;
  * grad_means: the forward's bound with g in place of x;  grad_rots: 8 u |gq|_1 (four products of a unit quaternion's entries
    with gq's, each chain rounding four times, quat(R) once).
"""
import math

import pytest
import torch

import object_motion_mirror as OM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
F64 = torch.float64
SIZES, OBJECTS = (1, 63, 64, 65, 257, 70001), (0, 1, 3, 16)
INTR_160 = dict(fx=133.9, fy=134.8, cx=80.3, cy=61.7, W=160, H=120)
INTR_64 = dict(fx=55.3, fy=54.1, cx=31.7, cy=24.3, W=64, H=48)


def _case(P, M, seed, mode="mixed"):
    """float32 CPU inputs.  ``mixed``: half the Gaussians carry a moving id, the rest any id (ids outside the moving ones are static);
    the LAST slot is held by no Gaussian when M >= 3 (an empty slot); ``static``: no Gaussian carries a moving id."""
    from monogs_amd import camera as cam
    g = torch.Generator().manual_seed(seed)
    R = torch.stack([cam.so3_exp(torch.randn(3, dtype=F64, generator=g) * 1.3) for _ in range(M)]).float() if M else torch.zeros(0, 3, 3)
    t = torch.randn(M, 3, generator=g)
    ids = torch.randperm(256, generator=g)[:M]
    table = torch.full((256,), -1, dtype=torch.int32)
    table[ids] = torch.arange(M, dtype=torch.int32)
    if M >= 2:
        table[int(torch.randperm(256, generator=g)[0])] = 99          # an entry outside 0..M-1 counts as static too (whichever id it hits)
        table[ids] = torch.arange(M, dtype=torch.int32)
    labels = torch.randint(0, 256, (P,), generator=g).to(torch.uint8)
    used = ids[:M - 1] if M >= 3 else ids
    if M and mode == "mixed":
        labels[::2] = used[torch.randint(0, len(used), ((P + 1) // 2,), generator=g)].to(torch.uint8)
    if M >= 3 or mode == "static":
        drop = ids[M - 1:] if mode == "mixed" else ids
        spare = [i for i in range(256) if int(table[i]) < 0][0]
        for i in drop.tolist():
            labels[labels == i] = spare
    x = torch.randn(P, 3, generator=g) * 2
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g))
    gx, gq = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g)
    return dict(P=P, M=M, R=R, t=t, table=table, labels=labels, x=x, q=q, gx=gx, gq=gq)


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _forward(lib, c, with_rot=True):
    from monogs_amd import _lib
    P, M = c["P"], c["M"]
    x, q, lab, tab, R, t = _d(c["x"]), _d(c["q"]) if with_rot else None, _d(c["labels"]), _d(c["table"]), _d(c["R"]), _d(c["t"])
    xo, qo = torch.full_like(x, float("nan")), torch.full_like(q, float("nan")) if with_rot else None
    p = lambda v: None if v is None or v.numel() == 0 else v.data_ptr()  # noqa: E731
    _lib.check(lib.mgs_object_transform_forward(P, M, p(lab), p(tab), p(R), p(t), p(x), p(q), p(xo), p(qo), None), "forward")
    torch.cuda.synchronize()
    return xo, qo


def _backward(lib, c, xo, qo, with_rot=True, perm=None):
    from monogs_amd import _lib
    P, M = c["P"], c["M"]
    sel = (lambda v: v) if perm is None else (lambda v: v[perm])
    lab, tab, R = _d(sel(c["labels"])), _d(c["table"]), _d(c["R"])
    gx, gq = _d(sel(c["gx"])), _d(sel(c["gq"])) if with_rot else None
    xo, qo = _d(sel(xo.cpu())), _d(sel(qo.cpu())) if with_rot else None
    dx, dq = torch.full_like(gx, float("nan")), torch.full_like(gq, float("nan")) if with_rot else None
    tau = torch.full((M, 6), float("nan"), device=DEV)
    scratch = torch.empty(lib.mgs_object_motion_scratch_bytes(P, M), dtype=torch.uint8, device=DEV)
    p = lambda v: None if v is None or v.numel() == 0 else v.data_ptr()  # noqa: E731
    _lib.check(lib.mgs_object_transform_backward(P, M, p(lab), p(tab), p(R), p(xo), p(qo), p(gx), p(gq), p(dx), p(dq), p(tau),
                                                 scratch.data_ptr(), None), "backward")
    torch.cuda.synchronize()
    return tau, dx, dq


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("M", OBJECTS)
def test_forward_against_the_mirror(native_lib, P, M):
    for mode, with_rot in (("mixed", True), ("mixed", False), ("static", True)):        # the last: all-static labels; the middle: rots = NULL
        _forward_case(native_lib, P, M, mode, with_rot)


def _forward_case(native_lib, P, M, mode, with_rot):
    c = _case(P, M, 100 + P + M, mode)
    xo, qo = _forward(native_lib, c, with_rot)
    mx, mq = OM.forward(c["x"], c["q"] if with_rot else None, c["labels"], c["table"], c["R"], c["t"])
    slot = OM.slots(c["labels"], c["table"], M)
    moved = slot >= 0
    assert mode == "static" or M == 0 or bool(moved.any())
    assert mode != "static" or not bool(moved.any())
    if M >= 3 and mode == "mixed":
        assert int((slot == M - 1).sum()) == 0                     # the empty slot
    xo_c = xo.cpu()
    assert torch.equal(xo_c[~moved], c["x"][~moved])               # static rows: bit for bit
    if with_rot:
        assert torch.equal(qo.cpu()[~moved], c["q"][~moved])
    if bool(moved.any()):
        s = slot[moved]
        bound = 4 * U * (c["x"][moved].double().abs().sum(1) + c["t"][s].double().abs().max(1).values)
        err = (xo_c[moved].double() - mx[moved]).abs().max(1).values
        print(f"forward P={P} M={M}: worst mean error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        if with_rot:
            eq = (qo.cpu()[moved].double() - mq[moved]).abs().max()
            print(f"forward P={P} M={M}: worst quaternion error {float(eq) / U:.2f} u")
            assert float(eq) <= 8 * U


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("M", OBJECTS)
def test_backward_against_the_mirror(native_lib, P, M):
    for with_rot in (True, False):
        _backward_case(native_lib, P, M, with_rot)


def _backward_case(native_lib, P, M, with_rot):
    c = _case(P, M, 100 + P + M)
    xo, qo = _forward(native_lib, c, with_rot)
    tau, dx, dq = _backward(native_lib, c, xo, qo, with_rot)
    gq = c["gq"] if with_rot else None
    m_tau, m_dx, m_dq = OM.backward(xo.cpu(), qo.cpu() if with_rot else None, c["labels"], c["table"], c["R"], c["gx"], gq)
    slot = OM.slots(c["labels"], c["table"], M)
    _, absn, counts = OM.closed_form_tau(xo.cpu(), qo.cpu() if with_rot else None, slot, M, c["gx"], gq)
    bound = (counts.double()[:, None] + 2) * U * absn
    err = (tau.cpu().double() - m_tau).abs()
    if M:
        print(f"backward P={P} M={M} rot={with_rot}: worst tau error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    for m in range(M):
        if int(counts[m]) == 0:
            assert bool((tau[m] == 0).all())                       # an empty slot: exactly 0
    b_x = 4 * U * c["gx"].double().abs().sum(1, keepdim=True)
    assert bool(((dx.cpu().double() - m_dx).abs() <= b_x).all())
    assert torch.equal(dx.cpu()[slot < 0], c["gx"][slot < 0])
    if with_rot:
        assert bool(((dq.cpu().double() - m_dq).abs() <= 8 * U * c["gq"].double().abs().sum(1, keepdim=True)).all())
        assert torch.equal(dq.cpu()[slot < 0], c["gq"][slot < 0])
    # two runs: bit-identical
    tau2, dx2, _ = _backward(native_lib, c, xo, qo, with_rot)
    assert torch.equal(tau, tau2) and torch.equal(dx, dx2)
    # the Gaussians permuted: within the same bound (order independence is not claimed)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(P))
    tau3, dx3, _ = _backward(native_lib, c, xo, qo, with_rot, perm=perm)
    assert bool(((tau3.cpu().double() - m_tau).abs() <= bound).all())
    assert torch.equal(dx3.cpu(), dx.cpu()[perm])


def _quat_mul(a, b):
    return OM.quat_mul(a, b)


def test_transform_objects_through_the_rasteriser(native_lib):
    """2 000 anisotropic Gaussians at 64 x 48, two moving objects: ``transform_objects`` -> rasteriser -> sum of squares against the
    same rasteriser fed by ``x @ R.T + t`` (and ``quat(R) (x) q``) written in torch, with ``exp(tau^)`` in front of it and ``tau = 0`` a
    leaf.  Same images; the op's pose gradients equal autograd's within (n_m + 2) u sum|term|."""
    from monogs_amd import camera as cam
    from monogs_amd.object_motion import ObjectPoses, transform_objects
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from monogs_amd.synthetic import make_scene, scene_settings
    sc = make_scene(2000, INTR_64, seed=7, anisotropic=True, near_fraction=0.0)
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    P = 2000
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 6, (P,), generator=g).to(torch.uint8).to(DEV)
    poses = ObjectPoses([4, 1], DEV)
    poses.set_pose(4, cam.so3_exp(torch.tensor([0.03, -0.05, 0.02])), [0.04, -0.02, 0.05])
    poses.set_pose(1, cam.so3_exp(torch.tensor([-0.02, 0.04, 0.06])), [-0.03, 0.03, -0.02])
    x, q = sc.means3D.to(DEV), sc.rotations.to(DEV)
    rest = dict(means2D=torch.zeros(P, 3, device=DEV), opacities=sc.opacities.to(DEV), colors_precomp=sc.colors.to(DEV),
                scales=sc.scales.to(DEV))

    def loss_of(xyz2, rot2):
        color, _, depth, _, _ = GaussianRasterizer(st)(means3D=xyz2, rotations=rot2, **rest)
        return (color ** 2).sum() + (depth ** 2).sum(), color.detach(), depth.detach()

    # ---- the op
    x2, q2 = transform_objects(x, q, labels, poses)
    x2.retain_grad(); q2.retain_grad()
    L, color, depth = loss_of(x2, q2)
    L.backward()
    g_theta, g_rho = poses.rot_delta.grad.clone(), poses.trans_delta.grad.clone()
    # ---- plain torch
    tau = torch.zeros(2, 6, device=DEV, requires_grad=True)
    slot = poses.slot_of_label[labels.long()].long()
    x1, q1 = x, q
    for m in range(2):
        th, rho = tau[m, 3:], tau[m, :3]
        K = torch.stack([torch.stack([th[0] * 0, -th[2], th[1]]), torch.stack([th[2], th[0] * 0, -th[0]]), torch.stack([-th[1], th[0], th[0] * 0])])
        xm = (x @ poses.R[m].t() + poses.T[m]) @ (torch.eye(3, device=DEV) + K).t() + rho          # exp(tau^) to first order: exact at tau = 0
        qe = torch.cat([torch.ones(1, device=DEV), 0.5 * th])
        qm = _quat_mul(qe.expand(P, 4), _quat_mul(OM.quat_of(poses.R[m].cpu()).float().to(DEV).expand(P, 4), q))
        x1 = torch.where((slot == m)[:, None], xm, x1)
        q1 = torch.where((slot == m)[:, None], qm, q1)
    Lr, color_r, depth_r = loss_of(x1, q1)
    Lr.backward()
    torch.cuda.synchronize()
    print(f"  images: colour differs by {float((color - color_r).abs().max()):.2e}, depth by {float((depth - depth_r).abs().max()):.2e}")
    assert (color - color_r).abs().max() <= 1e-3 and (depth - depth_r).abs().max() <= 1e-3        # (sanity: the same scene)
    _, absn, counts = OM.closed_form_tau(x2.detach().cpu(), q2.detach().cpu(), slot.cpu(), 2, x2.grad.cpu(), q2.grad.cpu())
    bound = (counts.double()[:, None] + 2) * U * absn
    got = torch.cat([g_rho, g_theta], 1).cpu().double()
    err = (got - tau.grad.cpu().double()).abs()
    print(f"through the rasteriser: objects of {counts.tolist()} Gaussians, worst pose-gradient error / bound {float((err / bound).max()):.3f}")
    print(f"  op {got.tolist()}\n  autograd {tau.grad.cpu().tolist()}")
    assert int(counts.min()) > 100
    assert bool((err <= bound).all()), (err / bound)


# ---- the dynamic room ------------------------------------------------------------------------------------------------------
N_FRAMES = 6


def _build_map(frame0, intr, bg):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    gmap = GaussianMap(DEV, nr_objects=19)
    frame0.update_RT(frame0.R_gt.clone(), frame0.T_gt.clone())
    gmap.extend_from_frame(frame0, intr, downsample=1, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([frame0], iters=80, init=True)
    return gmap


@pytest.fixture(scope="module")
def dynamic_room(native_lib):
    from monogs_amd.sequences import DYNAMIC_BOX_ID, make_dynamic_room_sequence
    frames, intr, object_poses = make_dynamic_room_sequence(N_FRAMES, INTR_160, DEV)
    bg = torch.zeros(3, device=DEV)
    gmap = _build_map(frames[0], intr, bg)
    n_box = int((frames[0].segmentation == DYNAMIC_BOX_ID).sum())
    print(f"dynamic room: {len(gmap)} Gaussians, the box covers {n_box} pixels of frame 0")
    assert n_box > 500
    return frames, intr, object_poses, bg, gmap


def _box_errors(run, object_poses):
    """Per frame 1..: (error of the previous frame's estimate against this frame's truth, error after tracking), metres, of the box centre."""
    from monogs_amd.object_motion import object_position_error
    from monogs_amd.sequences import DYNAMIC_BOX, DYNAMIC_BOX_ID
    centre = [0.5 * (a + b) for a, b in zip(*DYNAMIC_BOX)]
    est = run["objects"][DYNAMIC_BOX_ID]
    return [(object_position_error(est[i - 1], object_poses[i], centre), object_position_error(est[i], object_poses[i], centre))
            for i in range(1, len(est))]


def _ate(cams, frames):
    e = [float((-(R.t() @ t) + (f.R_gt.t() @ f.T_gt)).norm()) for (R, t), f in zip(cams[1:], frames[1:])]
    return math.sqrt(sum(v * v for v in e) / len(e))


def _quadrant_scene():
    """A map whose rasteriser gradients do not depend on the order of execution: four layers of one Gaussian per 8 x 8 quadrant of a
    64 x 48 image, each well inside its quadrant (screen variance 0.6 + 0.3 around the quadrant's centre: alpha is below 1/255 from
    3.5 pixels on, the quadrant's own border), all of object 1, seen from the identity pose; and a frame of it with the object moved
    by a tenth of a pixel.  Four layers of opacity 0.99: the tracking loss only counts pixels whose opacity exceeds 0.99 -- here the
    four in the middle of every quadrant."""
    from types import SimpleNamespace
    from monogs_amd.frames import Intrinsics, Viewpoint
    from monogs_amd.object_motion import ObjectPoses, ObjectTracker
    from monogs_amd import camera as cam
    k = INTR_64
    intr = Intrinsics(k, DEV)
    g = torch.Generator().manual_seed(4)
    qx, qy = torch.meshgrid(torch.arange(8.0), torch.arange(6.0), indexing="ij")
    px, py = (8 * qx + 3.5).reshape(-1).repeat(4), (8 * qy + 3.5).reshape(-1).repeat(4)
    z = torch.cat([torch.full((48,), 2.0 + 0.1 * layer) for layer in range(4)])
    xyz = torch.stack([(px + 0.5 - k["cx"]) * z / k["fx"], (py + 0.5 - k["cy"]) * z / k["fy"], z], 1)
    P = xyz.shape[0]
    gmap = SimpleNamespace(get_xyz=xyz.to(DEV), get_rotation=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1).to(DEV),
                           get_scaling=(math.sqrt(0.6) * z / k["fx"])[:, None].to(DEV), get_opacity=torch.full((P, 1), 0.99, device=DEV),
                           get_features=(0.2 + 0.6 * torch.rand(P, 3, generator=g)).to(DEV),
                           get_obj_prob=torch.tensor([[0.0, 1.0]]).repeat(P, 1).to(DEV))
    bg = torch.zeros(3, device=DEV)
    poses = ObjectPoses([1], DEV, lr_rot=0.0003, lr_trans=0.0003)       # (five steps stay below a tenth of a pixel: inside the quadrants)
    tracker = ObjectTracker(intr, gmap, bg, poses, border=0)
    # the frame: the map itself with the object at a known pose
    from monogs_amd.object_motion import MovedMap
    from monogs_amd.map_step import render_map
    poses.set_pose(1, cam.so3_exp(torch.tensor([0.0, 0.0, 0.001])), [0.003, -0.002, 0.004])
    vp0 = Viewpoint(1, torch.zeros(3, k["H"], k["W"], device=DEV), torch.ones(k["H"], k["W"], device=DEV), DEV)
    with torch.no_grad():
        pkg = render_map(vp0, intr, MovedMap(gmap, tracker.labels, poses), bg)
    seg = torch.ones(k["H"], k["W"], dtype=torch.int32, device=DEV)
    vp = Viewpoint(1, pkg["render"].detach().clone(), pkg["depth"][0].detach().clone(), DEV, segmentation=seg)
    poses.set_pose(1, torch.eye(3), torch.zeros(3))
    return tracker, poses, vp


def _five(tracker, poses, vp, obj_id, replayed):
    from monogs_amd import rasterizer as _r
    poses.set_pose(obj_id, torch.eye(3), torch.zeros(3))
    tracker.load(vp)
    if not replayed:
        for _ in range(5):
            tracker.iteration()
    else:
        graph, flags = torch.cuda.CUDAGraph(), _r.graph_flags()
        with flags, torch.cuda.graph(graph):
            tracker.iteration()
        assert torch.equal(poses.T, torch.zeros_like(poses.T))         # (a capture runs nothing; the state is still that of load())
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        assert not _r.check_overflow()
        flags.release()
    torch.cuda.synchronize()
    assert int(poses.t_dev[0]) == 5
    return poses.R.clone(), poses.T.clone()


def test_capture_of_one_tracker_iteration(dynamic_room):
    """One ``ObjectTracker`` iteration captured with ``torch.cuda.graph`` and replayed five times gives the poses of five eager
    iterations, bit for bit.  What this pull request adds is reproducible (the two-runs test above); the rasteriser's backward is
    not where three or more 8 x 8 quadrants add into one Gaussian's gradient line with float atomics in whatever order they run
    (tests/test_gpu_slam_contract.py: "two runs of one sequence are not bit-identical").  So the bitwise comparison is made on a map
    every Gaussian of which lies inside one quadrant (one add per line: no order).  The dynamic room is run as well and the
    difference REPORTED, not asserted: two runs of this test gave 1.9e-9 and 8.6e-6 in R, 0 and 2.1e-7 in T -- Adam's first steps are
    lr * g / |g|, so a gradient component near zero turns a last-bit difference into a different step."""
    from monogs_amd.frames import Viewpoint
    from monogs_amd.object_motion import ObjectPoses, ObjectTracker
    from monogs_amd.sequences import DYNAMIC_BOX_ID
    tracker, poses, vp = _quadrant_scene()
    eager = _five(tracker, poses, vp, 1, replayed=False)
    again = _five(tracker, poses, vp, 1, replayed=False)
    replay = _five(tracker, poses, vp, 1, replayed=True)
    print(f"capture, quadrant map: T eager {eager[1].tolist()} replayed {replay[1].tolist()}")
    assert float(eager[1].abs().max()) > 1e-4                          # the poses moved
    assert torch.equal(eager[0], again[0]) and torch.equal(eager[1], again[1])
    assert torch.equal(eager[0], replay[0]) and torch.equal(eager[1], replay[1])
    # the dynamic room, where the rasteriser's atomics are free to reorder
    frames, intr, object_poses, bg, gmap = dynamic_room
    f = frames[1]
    vp = Viewpoint(f.frame_idx, f.rgb, f.depth, DEV, gt_R=f.R_gt, gt_T=f.T_gt, segmentation=f.segmentation)
    vp.update_RT(f.R_gt.clone(), f.T_gt.clone())
    poses = ObjectPoses([DYNAMIC_BOX_ID], DEV)
    tracker = ObjectTracker(intr, gmap, bg, poses)
    eager = _five(tracker, poses, vp, DYNAMIC_BOX_ID, replayed=False)
    replay = _five(tracker, poses, vp, DYNAMIC_BOX_ID, replayed=True)
    dR, dT = float((eager[0] - replay[0]).abs().max()), float((eager[1] - replay[1]).abs().max())
    print(f"capture, dynamic room: eager T {eager[1].tolist()}, largest difference to the replays {dT:.3e} (R: {dR:.3e})")
    assert math.isfinite(dR) and math.isfinite(dT)


def test_tracking_the_box_with_the_ground_truth_camera(dynamic_room):
    from monogs_amd.object_motion import track_dynamic_sequence
    from monogs_amd.sequences import DYNAMIC_BOX_ID
    frames, intr, object_poses, bg, gmap = dynamic_room
    run = track_dynamic_sequence(frames, intr, gmap, bg, [DYNAMIC_BOX_ID], camera="gt", max_iters=100)
    errs = _box_errors(run, object_poses)
    print("gt camera: box (before, after) mm per frame:", [(round(a * 1e3, 2), round(b * 1e3, 2)) for a, b in errs], "iterations:", run["iters"])
    assert len(errs) == N_FRAMES - 1
    for i, (before, after) in enumerate(errs, 1):
        assert after < 0.5 * before, (i, before, after)
    assert all(1 < n < 100 for _, _, n in run["iters"]), run["iters"]


def test_tracking_the_box_with_the_tracked_camera(dynamic_room):
    """The camera's ATE against ``track_eager`` on the same sequence with the box held still and nothing masked: at most twice that
    plus 1.5 mm, the factor and the slack of tests/test_gpu_slam.py.  The unmasked run on the moving box is printed, not asserted."""
    from monogs_amd.frames import Viewpoint
    from monogs_amd.object_motion import track_dynamic_sequence
    from monogs_amd.sequences import DYNAMIC_BOX_ID, make_dynamic_room_sequence
    from monogs_amd.tracking import track_eager
    frames, intr, object_poses, bg, gmap = dynamic_room
    run = track_dynamic_sequence(frames, intr, gmap, bg, [DYNAMIC_BOX_ID], camera="track", max_iters=100)
    errs = _box_errors(run, object_poses)
    ate = _ate(run["camera"], frames)

    def plain(seq, the_map):                  # the camera alone, every pixel counted
        cams = [(seq[0].R_gt.clone(), seq[0].T_gt.clone())]
        for f in seq[1:]:
            vp = Viewpoint(f.frame_idx, f.rgb, f.depth, DEV, gt_R=f.R_gt, gt_T=f.T_gt)
            vp.update_RT(cams[-1][0].clone(), cams[-1][1].clone())
            track_eager(vp, intr, the_map, bg, 100)
            cams.append((vp.R.detach().clone(), vp.T.detach().clone()))
        return _ate(cams, seq)

    still, _, _ = make_dynamic_room_sequence(N_FRAMES, INTR_160, DEV, object_motion=lambda i: (torch.eye(3), torch.zeros(3)))
    ref = plain(still, _build_map(still[0], intr, bg))
    unmasked = plain(frames, gmap)
    print(f"tracked camera: box (before, after) mm per frame: {[(round(a * 1e3, 2), round(b * 1e3, 2)) for a, b in errs]} iterations: {run['iters']}")
    print(f"camera ATE: masked, box moving {ate * 1e3:.3f} mm | box still, nothing masked (the reference) {ref * 1e3:.3f} mm | "
          f"box moving, nothing masked {unmasked * 1e3:.3f} mm")
    for i, (before, after) in enumerate(errs, 1):
        assert after < 0.5 * before, (i, before, after)
    assert all(1 < n < 100 for _, _, n in run["iters"]), run["iters"]
    slack = 1.5e-3
    assert ate <= 2.0 * ref + slack, (ate, ref)
