"""Rigid object motion without a GPU: the float64 mirror (tests/object_motion_mirror.py) against the closed forms the kernels
implement, the retraction against ``cam.so3_exp`` composition, the argument checks of ``ObjectPoses``, ``frames.mask_objects`` and the
declarations of the three entry points."""
import os
import re

import pytest
import torch

import object_motion_mirror as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mgs_object_motion_scratch_bytes", "mgs_object_transform_forward", "mgs_object_transform_backward")
F64 = torch.float64


def _rot(g):
    from monogs_amd import camera as cam
    return cam.so3_exp(torch.randn(3, dtype=F64, generator=g) * 1.3)


def _case(P, M, seed, with_rot=True):
    g = torch.Generator().manual_seed(seed)
    R = torch.stack([_rot(g) for _ in range(M)]) if M else torch.zeros(0, 3, 3, dtype=F64)
    t = torch.randn(M, 3, dtype=F64, generator=g)
    table = torch.full((256,), -1, dtype=torch.int32)
    ids = torch.randperm(256, generator=g)[:M]
    table[ids] = torch.arange(M, dtype=torch.int32)
    labels = torch.randint(0, 256, (P,), generator=g).to(torch.uint8)
    if M:
        labels[::2] = ids[torch.randint(0, M, ((P + 1) // 2,), generator=g)].to(torch.uint8)
    x = torch.randn(P, 3, dtype=F64, generator=g) * 2
    q = torch.nn.functional.normalize(torch.randn(P, 4, dtype=F64, generator=g)) if with_rot else None
    gx = torch.randn(P, 3, dtype=F64, generator=g)
    gq = torch.randn(P, 4, dtype=F64, generator=g) if with_rot else None
    return R, t, table, labels, x, q, gx, gq


@pytest.mark.parametrize("P,M,with_rot", [(1, 1, True), (65, 3, True), (257, 16, True), (257, 3, False), (40, 0, True)])
def test_autograd_confirms_the_closed_forms(P, M, with_rot):
    R, t, table, labels, x, q, gx, gq = _case(P, M, 5 + P + M, with_rot)
    x_out, q_out = OM.forward(x, q, labels, table, R, t)
    g_tau, g_x, g_q = OM.backward(x_out, q_out, labels, table, R, gx, gq)
    slot = OM.slots(labels, table, M)
    tau, absn, counts = OM.closed_form_tau(x_out, q_out, slot, M, gx, gq)
    assert int(counts.sum()) == int((slot >= 0).sum())
    assert (g_tau - tau).abs().max() <= 1e-12 * max(1.0, float(absn.max())) if M else g_tau.numel() == 0
    # grad_means = R^T g for a moved Gaussian, g for a static one; grad_rots = conj(quat(R)) (x) gq
    want_x, want_q = gx.clone(), None if gq is None else gq.clone()
    for m in range(M):
        sel = slot == m
        want_x[sel] = gx[sel] @ R[m]
        if gq is not None:
            qc = OM.quat_of(R[m]) * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=F64)
            want_q[sel] = OM.quat_mul(qc.expand(int(sel.sum()), 4), gq[sel])
    assert (g_x - want_x).abs().max() <= 1e-12
    if gq is not None:
        assert (g_q - want_q).abs().max() <= 1e-12
    # the forward: static rows untouched, moved rows R x + t, and quat(R) (x) q turns a Gaussian as R does
    assert torch.equal(x_out[slot < 0], x[slot < 0])
    for m in range(M):
        sel = slot == m
        assert (x_out[sel] - (x[sel] @ R[m].t() + t[m])).abs().max() <= 1e-12 if bool(sel.any()) else True
        qr = OM.quat_of(R[m])
        assert abs(float(qr.norm()) - 1.0) < 1e-12


def _quat_to_R(q):
    r, x, y, z = (float(v) for v in q)
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                         [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                         [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=F64)


def test_quaternion_convention_is_the_rasterisers():
    """``R(quat(R_m) (x) q) = R_m R(q)`` with ``R(q)`` the rasteriser's ``(r, x, y, z)`` rotation matrix; every Shepperd branch."""
    from monogs_amd import camera as cam
    g = torch.Generator().manual_seed(2)
    thetas = [torch.randn(3, dtype=F64, generator=g) for _ in range(6)]
    thetas += [torch.tensor(v, dtype=F64) * 3.1 for v in ((1.0, 0.02, 0.01), (0.02, 1.0, 0.01), (0.01, 0.02, 1.0))]     # trace < 0
    for th in thetas:
        Rm = cam.so3_exp(th)
        q = torch.nn.functional.normalize(torch.randn(4, dtype=F64, generator=g), dim=0)
        assert (_quat_to_R(OM.quat_of(Rm)) - Rm).abs().max() < 1e-12
        assert (_quat_to_R(OM.quat_mul(OM.quat_of(Rm), q)) - Rm @ _quat_to_R(q)).abs().max() < 1e-12


def test_retraction_matches_so3_exp_composition():
    from monogs_amd import camera as cam
    g = torch.Generator().manual_seed(9)
    for scale in (1e-7, 1e-3, 0.4):
        R, t = _rot(g), torch.randn(3, dtype=F64, generator=g)
        rho, th = torch.randn(3, dtype=F64, generator=g) * scale, torch.randn(3, dtype=F64, generator=g) * scale
        R2, t2 = OM.retract(R, t, rho, th)
        dR = cam.so3_exp(th)
        assert (R2 - dR @ R).abs().max() < 1e-12
        assert (t2 - (dR @ t + cam.so3_left_jacobian(th) @ rho)).abs().max() < 1e-12
        Rn, tn, _ = cam.retract_pose(R, t, rho, th)
        assert (R2 - Rn).abs().max() < 1e-12 and (t2 - tn).abs().max() < 1e-12


def test_object_poses_argument_checks():
    from monogs_amd.object_motion import MAX_MOVING_OBJECTS, ObjectPoses
    assert MAX_MOVING_OBJECTS == 16
    for bad in ([256], [-1], [3, 3], list(range(17))):
        with pytest.raises(ValueError):
            ObjectPoses(bad, "cpu")
    p = ObjectPoses([18, 4], "cpu")
    assert p.M == 2 and p.slot_of_label.dtype == torch.int32 and p.slot_of_label.shape == (256,)
    assert int(p.slot_of_label[18]) == 0 and int(p.slot_of_label[4]) == 1 and int((p.slot_of_label >= 0).sum()) == 2
    assert torch.equal(p.R, torch.eye(3).repeat(2, 1, 1)) and torch.equal(p.T, torch.zeros(2, 3))
    assert p.rot_delta.shape == (2, 3) and p.trans_delta.requires_grad and p.lrs == (0.003, 0.001)
    R = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    p.set_pose(4, R, [1.0, 2.0, 3.0])
    assert torch.equal(p.pose(4)[0], R) and torch.equal(p.pose(4)[1], torch.tensor([1.0, 2.0, 3.0])) and torch.equal(p.pose(18)[0], torch.eye(3))
    with pytest.raises(KeyError):
        p.pose(5)
    p.m.fill_(1.0); p.t_dev.fill_(3)
    p.reset_optimizer()
    assert not p.m.any() and not p.t_dev.any()
    assert ObjectPoses([], "cpu").M == 0


def test_mask_objects_on_a_small_frame():
    from monogs_amd.frames import Viewpoint, mask_objects
    seg = torch.tensor([[0, 0, 5, 5], [0, 7, 5, 5], [0, 7, 7, 1], [1, 1, 1, 1]], dtype=torch.int32)
    rgb = torch.rand(3, 4, 4, generator=torch.Generator().manual_seed(1)) * 0.5 + 0.25
    depth = torch.full((4, 4), 2.0)
    mask = torch.ones(4, 4, dtype=torch.bool)
    mask[3, 3] = False
    vp = Viewpoint(3, rgb, depth, "cpu", gt_R=torch.eye(3), gt_T=torch.ones(3), mask=mask, segmentation=seg)
    vp.update_RT(torch.eye(3), torch.tensor([0.1, 0.2, 0.3]))
    dyn = (seg == 5) | (seg == 7)
    cam_view = mask_objects(vp, [5, 7])
    assert torch.equal(cam_view.mask, mask & ~dyn) and torch.equal(cam_view.depth, torch.where(dyn, torch.zeros(()), depth))
    obj_view = mask_objects(vp, [5, 7], keep=True)
    assert torch.equal(obj_view.mask, mask & dyn) and torch.equal(obj_view.depth, torch.where(dyn, depth, torch.zeros(())))
    for v in (cam_view, obj_view):
        assert v is not vp and v.frame_idx == 3 and torch.equal(v.T, vp.T) and v.T is not vp.T and v.rgb is vp.rgb
        assert torch.equal(v.grad_mask, vp.grad_mask) and v.segmentation is seg and torch.equal(v.T_gt, torch.ones(3))
        assert v.cam_rot_delta is not vp.cam_rot_delta
    # a border of one pixel: what is kept has nothing of the other side in its 3 x 3 neighbourhood (the image's edge is no side)
    assert mask_objects(vp, [5, 7], keep=True, border=1).mask.nonzero().tolist() == [[0, 3]]
    far = mask_objects(vp, [7], border=1)              # id 7 alone: the pixels two or more away from (1, 1), (2, 1), (2, 2)
    assert far.mask.nonzero().tolist() == [[0, 3]] and (far.depth > 0).nonzero().tolist() == [[0, 3]]
    # the original is untouched
    assert torch.equal(vp.mask, mask) and torch.equal(vp.depth, torch.full((4, 4), 2.0))
    assert not mask_objects(vp, []).mask[3, 3] and int(mask_objects(vp, []).mask.sum()) == 15
    with pytest.raises(ValueError, match="segmentation"):
        mask_objects(Viewpoint(0, rgb, depth, "cpu"), [5])


def test_header_and_binding_declare_the_entry_points():
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 26
    assert re.search(r"#define MGS_MAX_MOVING_OBJECTS 16\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        args = [a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[name][1]), (name, args)
    csrc = os.path.join(ROOT, "monogs_amd", "csrc")
    # a unit of its own: in the Makefile's SRCS, and included by nothing
    assert os.path.isfile(os.path.join(csrc, "object_motion.hip"))
    assert re.search(r"^SRCS\s*=.*\bobject_motion\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    units = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    assert not [f for f in units if re.search(r'#\s*include\s+"[^"]*object_motion\.\w+"', open(os.path.join(csrc, f)).read())]


def test_the_library_exports_them_and_refuses_bad_arguments(native_lib):
    for name in ENTRY_POINTS:
        assert hasattr(native_lib, name), name
    lib = native_lib
    assert lib.mgs_object_motion_scratch_bytes(0, 0) == 256 and lib.mgs_object_motion_scratch_bytes(-1, 1) == 256
    assert lib.mgs_object_motion_scratch_bytes(10, 17) == 256
    assert lib.mgs_object_motion_scratch_bytes(1025, 16) == 2 * 16 * 6 * 4          # two workgroups' rows
    assert lib.mgs_object_motion_scratch_bytes(70001, 3) == 5120                    # 69 rows x 3 x 6 floats = 4968 bytes, in 256s
    # refused before any launch (the pointers are never read: no device here)
    assert lib.mgs_object_transform_forward(8, 17, 0x100, 0x100, 0x100, 0x100, 0x100, None, 0x100, None, None) == 1
    assert b"moving objects" in lib.mgs_last_error()
    assert lib.mgs_object_transform_forward(8, 1, 0x100, None, 0x100, 0x100, 0x100, None, 0x100, None, None) == 1
    assert b"slot_of_label" in lib.mgs_last_error()
    assert lib.mgs_object_transform_forward(8, 1, 0x100, 0x100, 0x100, 0x100, 0x100, 0x100, 0x100, None, None) == 1
    assert lib.mgs_object_transform_backward(8, 17, 0x100, 0x100, 0x100, 0x100, None, 0x100, None, None, None, 0x100, 0x100, None) == 1
    assert lib.mgs_object_transform_backward(8, 1, 0x100, None, 0x100, 0x100, None, 0x100, None, None, None, 0x100, 0x100, None) == 1
    assert lib.mgs_object_transform_backward(8, 1, 0x100, 0x100, 0x100, 0x100, None, 0x100, None, None, 0x100, 0x100, 0x100, None) == 1
    assert lib.mgs_object_transform_backward(8, 1, 0x100, 0x100, 0x100, 0x100, None, 0x100, None, None, None, None, 0x100, None) == 1
