"""Pose-tangent rendering (csrc/pose_tangent.hip, ``pose_jacobian``), the normal equations and the Gauss-Newton step
(csrc/gauss_newton.hip, ``normal_equations``, ``PoseGaussNewton``) on the GPU.

Reference of the Jacobian: the float64 oracle by the double-backward construction (tests/pose_jacobian_mirror.py, checked without a
GPU in tests/test_pose_jacobian_host.py).  Per plane, on the pixels the oracle does not flag ambiguous in float64 or in float32,
    |J - J64| <= 1e-3 |J64| + f 1e-5 max_plane |J64|,     f = max(1, 4 r32),
r32 the float32 oracle's own worst ratio to the f = 1 bound on the scene (computed here): the factor 4 is the allowance for a
different, equally valid float32 evaluation (prescaled conic, exp2, hardware reciprocal).  At most 0.1 % of a scene's pixels may be
skipped.  The adjoint identity ties the planes to the HIP backward by the project's gradient rule with no outliers."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import intrinsics_scenes as S
import pose_jacobian_mirror as M
from monogs_amd.debug import options
from monogs_amd.synthetic import make_scene, scene_settings
from oracle import OracleSettings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.float64
NAMES = [n for n in S.SCENES if n != "sh2_257"] + ["capped"]
K70 = dict(fx=58.6, fy=59.0, cx=35.2, cy=25.9, W=70, H=50)
K9 = dict(fx=7.5, fy=7.6, cx=4.4, cy=3.6, W=9, H=7)


def _inputs(sc):
    scales = sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)
    return dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=scales, rotations=sc.rotations)


def _on_pixel_centres(sc, P, seed):
    """Camera-space points that project onto pixel centres, moved to the world of ``sc``'s pose."""
    k = sc.intr
    g = torch.Generator().manual_seed(seed)
    px = torch.randint(4, k["W"] - 4, (P,), generator=g).float()
    py = torch.randint(4, k["H"] - 4, (P,), generator=g).float()
    z = 1.0 + 3.0 * torch.rand(P, generator=g)
    pc = torch.stack([(px + 0.5 - k["cx"]) * z / k["fx"], (py + 0.5 - k["cy"]) * z / k["fy"], z], 1)
    return ((pc - sc.t[None, :]) @ sc.R).contiguous()


@functools.lru_cache(maxsize=None)
def _capped_scene():
    """Opacity 0.999 and centres on pixel centres: alpha is capped at 0.99 around every centre (the straight-through rule).  An integer
    centre and an integer radius can put a rectangle's edge exactly on a tile boundary, where float32 and float64 round to different
    tiles -- a decision the oracle does not flag; the seed is one for which both agree on every rectangle (_mirror_of asserts it)."""
    sc = make_scene(40, S.K64, seed=21, anisotropic=True, near_fraction=0.0, mean_radius_px=4.0)
    return sc._replace(means3D=_on_pixel_centres(sc, 40, 25), opacities=torch.full((40, 1), 0.999))


@functools.lru_cache(maxsize=None)
def _stack_scene():
    """Stacks that terminate early: per stack 24 faint splats in front of four wide opaque ones (alpha >= 0.9 within 3.7 px of the
    centre: the fourth would take T below 1e-4, so the pixel stops in front of it) and seven more behind, which no stopped pixel may
    take into S."""
    sc = make_scene(4 * 35, S.K64, seed=31, near_fraction=0.0, pose_tau=(0.0,) * 6)
    k = S.K64
    g = torch.Generator().manual_seed(32)
    means, opac, scale = [], [], []
    for cx_, cy_ in ((12.0, 12.0), (40.0, 10.0), (20.0, 36.0), (50.0, 34.0)):
        for i in range(35):
            z = 1.0 + 0.05 * i
            off = 3.0 * (torch.rand(2, generator=g) - 0.5) if not 24 <= i < 28 else torch.zeros(2)      # the opaque ones: centred
            means.append([(cx_ + off[0].item() + 0.5 - k["cx"]) * z / k["fx"], (cy_ + off[1].item() + 0.5 - k["cy"]) * z / k["fy"], z])
            opac.append(0.04 if i < 24 else (0.999 if i < 28 else 0.6))
            scale.append((8.0 if 24 <= i < 28 else 3.0) * z / k["fx"])
    return sc._replace(means3D=torch.tensor(means), opacities=torch.tensor(opac)[:, None], scales=torch.tensor(scale)[:, None],
                       rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(len(means), 1))


def _fixture(name):
    if name == "capped":
        sc = _capped_scene()
        return sc, _inputs(sc)
    sc, inp, _ = S.fixture(name)
    return sc, inp


@functools.lru_cache(maxsize=None)
def _mirror_of(key):
    """(J64, skip [H, W], f, r32) of a scene; computed once, never modified."""
    sc, inp = _SCENES[key]()
    st = scene_settings(sc, OracleSettings)
    J64, o64 = M.oracle_jacobian(inp, st, D, want_ambiguous=True)
    J32, o32 = M.oracle_jacobian(inp, st, torch.float32, want_ambiguous=True)
    skip = o64.aux["ambiguous"] | o32.aux["ambiguous"]
    if key == "capped":
        g64, g32 = o64.aux["geom"], o32.aux["geom"]
        assert torch.equal(g64["rect_min"], g32["rect_min"]) and torch.equal(g64["rect_max"], g32["rect_max"]), "wrong fixture"
    r32 = _worst_ratio(J32.to(D), J64, skip, 1.0)
    return J64, skip, max(1.0, 4.0 * r32), r32


def _worst_ratio(J, J64, skip, f):
    worst = 0.0
    for k in range(6):
        for c in range(5):
            ref = J64[k, c]
            top = ref.abs().max().item()
            if top == 0.0:
                assert (J[k, c][~skip] == 0).all(), (k, c)
                continue
            bound = 1e-3 * ref.abs() + f * 1e-5 * top
            worst = max(worst, ((J[k, c] - ref).abs() / bound)[~skip].max().item())
    return worst


_SCENES = {n: functools.partial(_fixture, n) for n in NAMES}
_SCENES["edge70"] = lambda: (lambda sc: (sc, _inputs(sc)))(make_scene(300, K70, seed=41, anisotropic=True, near_fraction=0.0, mean_radius_px=4.0))
_SCENES["edge9"] = lambda: (lambda sc: (sc, _inputs(sc)))(make_scene(12, K9, seed=42, near_fraction=0.0, mean_radius_px=2.0))
_SCENES["bg"] = lambda: (lambda sc: (sc, _inputs(sc)))(make_scene(300, S.K64, seed=43, anisotropic=True, near_fraction=0.0,
                                                                    mean_radius_px=4.0, bg=(0.3, 0.5, 0.7)))
_SCENES["stack"] = lambda: (lambda sc: (sc, _inputs(sc)))(_stack_scene())


def _forward(sc, inp):
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    t = {k: v.to(DEV) for k, v in inp.items()}
    theta, rho = torch.zeros(3, device=DEV, requires_grad=True), torch.zeros(3, device=DEV, requires_grad=True)
    color, radii, depth, opacity, _ = GaussianRasterizer(st)(
        means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
        colors_precomp=t.get("colors_precomp"), scales=t.get("scales"), rotations=t.get("rotations"),
        cov3D_precomp=t.get("cov3D_precomp"), theta=theta, rho=rho)
    return SimpleNamespace(color=color, depth=depth, opacity=opacity, theta=theta, rho=rho, radii=radii)


def _check_mirror(key, J, label=None):
    J64, skip, f, r32 = _mirror_of(key)
    n_skip, n_pix = int(skip.sum()), skip.numel()
    worst = _worst_ratio(J.detach().cpu().to(D), J64, skip, f)
    print(f"{label or key}: HIP worst ratio {worst:.3f} of the bound (f = {f:.2f}, r32 = {r32:.3f}, skipped {n_skip} of {n_pix} pixels)")
    assert n_skip <= 1e-3 * n_pix, (n_skip, n_pix)
    assert worst <= 1.0, (key, worst)


def _check_adjoint(key, fw, J):
    sc, _ = _SCENES[key]()
    gc, gd = sc.grad_color.to(DEV), sc.grad_depth.to(DEV)
    ((fw.color * gc).sum() + (fw.depth * gd).sum()).backward()
    ref = torch.cat([fw.rho.grad, fw.theta.grad]).cpu()
    got = (J[:, :4].double() * torch.cat([gc, gd], 0).double()[None]).sum(dim=(1, 2, 3)).cpu()
    ok, worst = S.rel_rule(got, ref)
    print(f"{key}: adjoint identity {worst:.3f} of the bound; dL/dtau {ref.tolist()}")
    assert ok, (got, ref)


# ---- 1. against the mirror, 2. the adjoint identity against the HIP backward ---------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_jacobian_against_the_mirror_and_the_backward(native_lib, name):
    from monogs_amd.pose_jacobian import pose_jacobian
    sc, inp = _SCENES[name]()
    fw = _forward(sc, inp)
    J = pose_jacobian(fw.color)
    assert J.shape == (6, 5, sc.intr["H"], sc.intr["W"])
    _check_mirror(name, J)
    _check_adjoint(name, fw, J)
    if name == "capped":
        o = fw.opacity.detach()
        assert (o >= 0.99 - 1e-6).sum().item() >= 20          # the cap is hit where the centres sit


# ---- 3. seams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["edge70", "edge9", "bg", "stack"])
def test_seams_of_the_image_and_of_the_walk(native_lib, key):
    from monogs_amd.pose_jacobian import pose_jacobian
    sc, inp = _SCENES[key]()
    fw = _forward(sc, inp)
    J = pose_jacobian(fw.color)
    _check_mirror(key, J)
    _check_adjoint(key, fw, J)
    if key == "stack":
        assert (fw.opacity.detach() > 0.999).sum().item() >= 40              # pixels the forward stopped in front of the list's end


def test_binning_paths_and_capacity_mode(native_lib):
    from monogs_amd import rasterizer as R
    from monogs_amd.pose_jacobian import pose_jacobian
    sc, inp = _SCENES["aniso2000"]()
    P, W, H = inp["means3D"].shape[0], sc.intr["W"], sc.intr["H"]
    R.set_sync_free(False)
    assert native_lib.mgs_binning_path(P, W, H) == 0
    fw = _forward(sc, inp)
    ref = pose_jacobian(fw.color)
    _check_mirror("aniso2000", ref, "global depth sort")
    with options(radix_scanned=1):
        assert native_lib.mgs_binning_path(P, W, H) == 1
        fw1 = _forward(sc, inp)
        J1 = pose_jacobian(fw1.color)
    _check_mirror("aniso2000", J1, "per-tile depth sort")
    _check_adjoint("aniso2000", fw1, J1)
    try:
        R.set_sync_free(True, headroom=1.5)
        fw2 = _forward(sc, inp)
        assert fw2.color.grad_fn.overflow is not None          # the capacity path ran: the list's tail is never read
        J2 = pose_jacobian(fw2.color)
        assert not R.check_overflow()
    finally:
        R.set_sync_free(False)
        R.forget_capacity(P, W, H)
    _check_mirror("aniso2000", J2, "capacity mode")
    _check_adjoint("aniso2000", fw2, J2)


# ---- 4. exact zeros ----------------------------------------------------------------------------------------------------------
def test_exact_zeros(native_lib):
    from monogs_amd.pose_jacobian import pose_jacobian
    sc, inp = _SCENES["iso257"]()
    pc = inp["means3D"] @ sc.R.t() + sc.t[None, :]
    pc[:, 2] = -pc[:, 2].abs() - 0.5
    behind = dict(inp, means3D=((pc - sc.t[None, :]) @ sc.R).contiguous())
    J = pose_jacobian(_forward(sc, behind).color)
    assert J.shape == (6, 5, 48, 64) and (J == 0).all()
    empty = {k: v[:0].contiguous() for k, v in inp.items()}
    J0 = torch.full((6, 5, 48, 64), 7.0, device=DEV)
    J0.copy_(pose_jacobian(_forward(sc, empty).color))
    assert (J0 == 0).all()


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------
def test_reproducible_and_read_only(native_lib):
    from monogs_amd.pose_jacobian import pose_jacobian
    sc, inp = _SCENES["aniso2000"]()
    fw = _forward(sc, inp)
    assert torch.equal(pose_jacobian(fw.color), pose_jacobian(fw.color))
    q = S.quadrant_scene()
    qi = _inputs(q)
    gc, gd = q.grad_color.to(DEV), q.grad_depth.to(DEV)

    def run(with_jacobian):
        f = _forward(q, qi)
        if with_jacobian:
            pose_jacobian(f.color)
        ((f.color * gc).sum() + (f.depth * gd).sum()).backward()
        return [f.color.detach().clone(), f.depth.detach().clone(), f.opacity.detach().clone(), f.theta.grad.clone(), f.rho.grad.clone()]
    a, b = run(False), run(True)
    assert a[3].abs().min().item() > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 6. normal equations -------------------------------------------------------------------------------------------------------
def _frame(H, W, seed, J=None, images=None):
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    if images is None:
        color, depth = U(3, H, W), 0.5 + 3 * U(1, H, W)
        opacity = torch.where(U(1, H, W) < 0.8, torch.ones(1, H, W), U(1, H, W))
    else:
        color, depth, opacity = images
    vp = SimpleNamespace(rgb=(color + 0.2 * (U(3, H, W) - 0.5)).clamp(0, 1), depth=torch.where(U(H, W) < 0.85, depth[0] + 0.3 * (U(H, W) - 0.5), torch.zeros(H, W)),
                         mask=U(H, W) < 0.9, grad_mask=U(H, W) < 0.6, exposure_a=torch.tensor([0.07]), exposure_b=torch.tensor([-0.02]))
    if J is None:
        J = 4 * (U(6, 5, H, W) - 0.5)
    return J, color, depth, opacity, vp


def _check_system(J, color, depth, opacity, vp, d_rgb=0.05, d_depth=0.05, rgb_only=False, label=""):
    from monogs_amd.pose_jacobian import normal_equations
    dv = SimpleNamespace(**{k: v.to(DEV) for k, v in vars(vp).items()})
    args = (J.to(DEV), color.to(DEV), depth.to(DEV), opacity.to(DEV), dv)
    sy = normal_equations(*args, delta_rgb=d_rgb, delta_depth=d_depth, rgb_only=rgb_only)
    again = normal_equations(*args, delta_rgb=d_rgb, delta_depth=d_depth, rgb_only=rgb_only)
    assert torch.equal(sy.buf, again.buf)                        # bitwise reproducible
    H64, g64, E64, n_rgb, n_d = M.normal_equations(J, color, depth, opacity, vp.rgb, vp.depth, vp.mask, vp.grad_mask,
                                                   vp.exposure_a.item(), vp.exposure_b.item(), d_rgb, d_depth, rgb_only)
    Hh, gh, buf = sy.H.cpu(), sy.g.cpu(), sy.buf.cpu()
    assert torch.isfinite(buf).all()
    assert int(buf[73]) == n_rgb and int(buf[74]) == n_d, (buf[73:], n_rgb, n_d)
    dg = H64.diagonal().clamp_min(0).sqrt()
    tol_H = 1e-6 * dg[:, None] * dg[None, :]
    tol_g = 1e-6 * dg * (2 * E64) ** 0.5
    print(f"{label}: N_rgb {n_rgb} N_d {n_d} E {E64:.6e}; worst H {((Hh - H64).abs() / tol_H.clamp_min(1e-300)).max().item():.3e} "
          f"g {((gh - g64).abs() / tol_g.clamp_min(1e-300)).max().item():.3e} of the bound")
    assert ((Hh - H64).abs() <= tol_H).all()
    assert ((gh - g64).abs() <= tol_g).all()
    assert abs(buf[72].item() - E64) <= 1e-6 * E64
    assert torch.equal(Hh, Hh.t())
    return sy, (H64, g64, E64)


@pytest.mark.parametrize("size", [(48, 64), (50, 70), (1, 1)])
def test_normal_equations_on_random_planes(native_lib, size):
    H, W = size
    J, color, depth, opacity, vp = _frame(H, W, 60 + H)
    if (H, W) == (1, 1):
        opacity[:] = 1.0
        vp.mask[:], vp.grad_mask[:] = True, True
        vp.depth[:] = depth[0] + 0.1
    _check_system(J, color, depth, opacity, vp, label=f"random {W}x{H}")
    _check_system(J, color, depth, opacity, vp, rgb_only=True, label=f"random {W}x{H} rgb-only")
    _check_system(J, color, depth, opacity, vp, d_rgb=10.0, d_depth=10.0, label=f"random {W}x{H} quadratic")


def test_normal_equations_on_rendered_planes_and_the_empty_cases(native_lib):
    from monogs_amd.pose_jacobian import pose_jacobian
    sc, inp = _SCENES["aniso2000"]()
    fw = _forward(sc, inp)
    Jh = pose_jacobian(fw.color).cpu()
    images = (fw.color.detach().cpu(), fw.depth.detach().cpu(), fw.opacity.detach().cpu())
    J, color, depth, opacity, vp = _frame(48, 64, 71, J=Jh, images=images)
    _check_system(J, color, depth, opacity, vp, label="rendered")
    # all-masked: zeros, never NaN
    vp0 = SimpleNamespace(**dict(vars(vp), mask=torch.zeros(48, 64, dtype=torch.bool), depth=torch.zeros(48, 64)))
    sy, _ = _check_system(J, color, depth, opacity, vp0, label="all-masked")
    assert (sy.buf == 0).all()
    # N_d = 0 with colour rows
    vp1 = SimpleNamespace(**dict(vars(vp), depth=torch.zeros(48, 64)))
    sy, _ = _check_system(J, color, depth, opacity, vp1, label="N_d = 0")
    assert sy.n_depth.item() == 0 and sy.n_rgb.item() > 0
    # a residual exactly at delta: omega = 1 on that row
    one = lambda v: torch.full((1, 1, 1), v)  # noqa: E731
    vpd = SimpleNamespace(rgb=torch.full((3, 1, 1), 0.25), depth=torch.full((1, 1), 1.5), mask=torch.ones(1, 1, dtype=torch.bool),
                          grad_mask=torch.ones(1, 1, dtype=torch.bool), exposure_a=torch.zeros(1), exposure_b=torch.zeros(1))
    Jd = torch.arange(30, dtype=torch.float32).reshape(6, 5, 1, 1) / 7 + 0.1
    sy, (H64, _, E64) = _check_system(Jd, torch.full((3, 1, 1), 0.5), one(2.0), one(1.0), vpd, d_rgb=0.25, d_depth=0.5, label="at delta")
    assert abs(E64 - (3 * 0.5 / 3 * 0.5 * 0.25 ** 2 + 0.5 * 0.5 ** 2)) < 1e-15          # both rows on the quadratic branch


# ---- 7. the step ---------------------------------------------------------------------------------------------------------------
def _system_tensor(H, g, E=0.25):
    buf = torch.zeros(75, dtype=D)
    buf[:64], buf[64:72], buf[72] = H.reshape(-1), g, E
    return buf.to(DEV)


def _viewpoint(seed=5):
    from monogs_amd.camera import se3_exp
    from monogs_amd.frames import Viewpoint
    vp = Viewpoint(0, torch.zeros(3, 4, 4, device=DEV), torch.ones(4, 4, device=DEV), DEV, grad_mask=torch.ones(4, 4, dtype=torch.bool, device=DEV))
    T = se3_exp(torch.tensor([0.3, -0.1, 0.2, 0.2, -0.4, 0.1]))
    vp.update_RT(T[:3, :3].clone(), T[:3, 3].clone())
    with torch.no_grad():
        vp.exposure_a.fill_(0.03); vp.exposure_b.fill_(-0.01)
    return vp


def _spd(seed, scale):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(8, 12, generator=g, dtype=D)
    return A @ A.t(), scale * torch.randn(8, generator=g, dtype=D)


@pytest.mark.parametrize("fix_exposure", [False, True])
def test_step_against_the_mirror(native_lib, fix_exposure):
    from monogs_amd import camera as cam
    from monogs_amd.frames import Intrinsics
    from monogs_amd.pose_optim import PoseGaussNewton
    H, g = _spd(80, 0.02)
    vp = _viewpoint()
    R0, T0 = vp.R.cpu(), vp.T.cpu()
    intr = Intrinsics(S.K64, DEV)
    cam3 = (torch.empty(4, 4, device=DEV), torch.empty(4, 4, device=DEV), torch.empty(3, device=DEV))
    opt = PoseGaussNewton(vp, lam=1e-3, lam_abs=1e-6, max_rot=0.05, max_trans=0.05, fix_exposure=fix_exposure)
    conv = opt.step_and_retract(_system_tensor(H, g), camera=(intr.projection_matrix,) + cam3)
    Rm, Tm, am, bm, tn, ok = M.gn_step(H, g, R0, T0, 0.03, -0.01, 1e-3, 1e-6, 0.05, 0.05, fix_exposure)
    out = opt.out.cpu()
    assert ok and out[3].item() == 0 and not conv and abs(out[1].item() - tn) <= 1e-6 and abs(out[2].item() - 0.25) < 1e-7
    assert 1e-4 < tn < 0.05 * 2 ** 0.5
    assert (vp.R.cpu().double() - Rm).abs().max() <= 1e-6 and (vp.T.cpu().double() - Tm).abs().max() <= 1e-6
    assert abs(vp.exposure_a.item() - am) <= 1e-6 and abs(vp.exposure_b.item() - bm) <= 1e-6
    if fix_exposure:
        assert vp.exposure_a.item() == np.float32(0.03) and vp.exposure_b.item() == np.float32(-0.01)
    ref = cam.fused_camera_matrices(vp.R, vp.T, intr.projection_matrix)
    for x, y in zip(cam3, ref):
        assert torch.equal(x, y)                                  # bit-identical to mgs_camera_setup on the new pose
    assert torch.equal(opt.information().cpu(), H[:6, :6])


def test_step_failure_sticky_and_clamp(native_lib):
    from monogs_amd.pose_optim import PoseGaussNewton
    vp = _viewpoint()
    keep = [vp.R.clone(), vp.T.clone(), vp.exposure_a.data.clone(), vp.exposure_b.data.clone()]
    same = lambda: all(torch.equal(x, y) for x, y in zip(keep, [vp.R, vp.T, vp.exposure_a.data, vp.exposure_b.data]))  # noqa: E731
    # H = 0: status 1 and nothing moved
    opt = PoseGaussNewton(vp, lam=1e-3, lam_abs=0.0)
    assert not opt.step_and_retract(_system_tensor(torch.zeros(8, 8, dtype=D), torch.ones(8, dtype=D)))
    assert opt.out[3].item() == 1 and same()
    # an indefinite and a NaN system
    Hn, g = _spd(81, 0.02)
    Hn[2, 2] = -1.0
    assert not opt.step_and_retract(_system_tensor(Hn, g)) and opt.out[3].item() == 1 and same()
    Hn[2, 2] = float("nan")
    assert not opt.step_and_retract(_system_tensor(Hn, g)) and opt.out[3].item() == 1 and same()
    # the clamp: a large step is scaled as a whole
    H, g = _spd(82, 50.0)
    opt = PoseGaussNewton(vp, lam=0.0, lam_abs=0.0, max_rot=0.01, max_trans=0.02)
    R0, T0 = vp.R.cpu(), vp.T.cpu()
    opt.step_and_retract(_system_tensor(H, g))
    x = np.linalg.solve(H.numpy(), -g.numpy())
    assert np.linalg.norm(x[3:6]) > 0.01 and np.linalg.norm(x[:3]) > 0.02
    Rm, Tm, am, bm, tn, ok = M.gn_step(H, g, R0, T0, 0.03, -0.01, 0.0, 0.0, 0.01, 0.02)
    sc = min(0.01 / np.linalg.norm(x[3:6]), 0.02 / np.linalg.norm(x[:3]))
    assert abs(tn - sc * np.linalg.norm(x[:6])) < 1e-12 and abs(opt.out[1].item() - tn) <= 1e-6
    assert (vp.R.cpu().double() - Rm).abs().max() <= 1e-6 and (vp.T.cpu().double() - Tm).abs().max() <= 1e-6
    assert abs(vp.exposure_a.item() - am) <= 1e-6 and abs(vp.exposure_b.item() - bm) <= 1e-6
    # sticky: a second call after convergence is a no-op
    H, g = _spd(83, 1e-7)
    opt = PoseGaussNewton(vp, lam=0.0, lam_abs=0.0, sticky=True)
    flag = torch.zeros(1).pin_memory()
    assert opt.step_and_retract(_system_tensor(H, g), host_flag=flag)
    torch.cuda.synchronize()
    assert flag.item() == 1.0
    keep = [vp.R.clone(), vp.T.clone(), vp.exposure_a.data.clone(), vp.exposure_b.data.clone()]
    H2, g2 = _spd(84, 0.02)
    assert opt.step_and_retract(_system_tensor(H2, g2)) and same()
    opt.reset()
    assert not opt.step_and_retract(_system_tensor(H2, g2)) and not same()


# ---- 8. Gauss-Newton consistency ---------------------------------------------------------------------------------------------
def test_gauss_newton_consistency(native_lib):
    """Target rendered from the true pose, the viewpoint 5 mm / 0.3 degrees away, deltas large (omega = 1): g[:6] is the HIP backward's
    dL/dtau of the matching quadratic loss, and one undamped step more than halves the pose error."""
    from monogs_amd.camera import se3_exp
    from monogs_amd.frames import Viewpoint
    from monogs_amd.pose_jacobian import normal_equations, pose_jacobian
    from monogs_amd.pose_optim import PoseGaussNewton
    sc, inp = _SCENES["aniso2000"]()
    true = _forward(sc, inp)
    rho, theta = torch.tensor([0.6, -0.6, 0.52]), torch.tensor([0.57, -0.58, 0.58])
    d = torch.cat([0.005 * rho / rho.norm(), float(np.radians(0.3)) * theta / theta.norm()])          # 5 mm, 0.3 degrees
    Tn = se3_exp(d) @ torch.cat([torch.cat([sc.R, sc.t[:, None]], 1), torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    moved = sc._replace(R=Tn[:3, :3].contiguous(), t=Tn[:3, 3].contiguous())
    H, W = sc.intr["H"], sc.intr["W"]
    vp = Viewpoint(0, true.color.detach().clone(), true.depth.detach()[0].clone(), DEV,
                   gt_R=sc.R.to(DEV), gt_T=sc.t.to(DEV), grad_mask=torch.ones(H, W, dtype=torch.bool, device=DEV))
    vp.update_RT(moved.R.clone(), moved.t.clone())
    fw = _forward(moved, inp)
    J = pose_jacobian(fw.color)
    sy = normal_equations(J, fw.color, fw.depth, fw.opacity, vp, delta_rgb=1e3, delta_depth=1e3)
    # the matching quadratic loss: sum s 0.5 r^2 over the same rows
    with torch.no_grad():
        sat = fw.opacity[0] > 0.99
        m_rgb, m_d = sat, sat & (vp.depth > 0)
        d_color = torch.where(m_rgb[None], (fw.color - vp.rgb) * (0.5 / (3 * H * W)), torch.zeros_like(fw.color))
        d_depth = torch.where(m_d[None], (fw.depth - vp.depth[None]) / m_d.sum(), torch.zeros_like(fw.depth))
    torch.autograd.backward([fw.color, fw.depth], [d_color, d_depth])
    ref = torch.cat([fw.rho.grad, fw.theta.grad]).cpu()
    ok, worst = S.rel_rule(sy.g[:6].cpu(), ref)
    print(f"g[:6] against the backward: {worst:.3f} of the bound; g {sy.g[:6].tolist()}")
    assert ok, (sy.g[:6], ref)

    def err():
        c = -(vp.R.t() @ vp.T).cpu() + (sc.R.t() @ sc.t)
        ang = torch.arccos((((vp.R.cpu() @ sc.R.t()).trace() - 1) / 2).clamp(-1, 1))
        return (c.norm() ** 2 + ang ** 2).sqrt().item()
    e0 = err()
    opt = PoseGaussNewton(vp, lam=0.0, lam_abs=0.0, max_rot=1.0, max_trans=1.0, fix_exposure=True)
    opt.step_and_retract(sy)
    e1 = err()
    print(f"pose error {e0:.3e} -> {e1:.3e}")
    assert opt.out[3].item() == 0 and e1 < 0.5 * e0
    info = opt.information()
    assert torch.linalg.eigvalsh(info.cpu()).min().item() > 0
