"""The intrinsics gradient of the HIP backward (MGS_FLAG_INTRINSICS_GRAD, ``GaussianRasterizer(..., intr=delta)``) and the calibration
loop built on it, on the GPU.  The reference of the gradient is the float64 oracle's central differences (tests/intrinsics_scenes.py;
tests/test_intrinsics_host.py checks that reference without a GPU); the bar is the project's elementwise gradient rule
(tests/test_gpu_parity.py::_check_grads, north_star's 1e-3) with no outliers."""
from types import SimpleNamespace

import pytest
import torch

import intrinsics_scenes as S
from monogs_amd.synthetic import make_scene, scene_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(sc, inp, deg=0, intr=True, second_backward=False, pose=True):
    """One forward + backward of ``<g_c, colour> + <g_d, depth>`` through the public rasteriser.  Returns a dict of CPU gradients;
    ``second_backward``: also those of a second backward through the same forward (the unprepared scratch), under ``"second"``."""
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV, sh_degree=deg)
    leaves = {k: v.to(DEV).clone().requires_grad_(True) for k, v in inp.items()}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    extra = {}
    if pose:
        extra.update(theta=torch.zeros(3, device=DEV, requires_grad=True), rho=torch.zeros(3, device=DEV, requires_grad=True))
    if intr:
        extra["intr"] = torch.zeros(4, device=DEV, requires_grad=True)
    color, radii, depth, _, _ = GaussianRasterizer(st)(
        means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves.get("shs"),
        colors_precomp=leaves.get("colors_precomp"), scales=leaves.get("scales"), rotations=leaves.get("rotations"),
        cov3D_precomp=leaves.get("cov3D_precomp"), **extra)
    loss = (color * sc.grad_color.to(DEV)).sum() + (depth * sc.grad_depth.to(DEV)).sum()

    def collect():
        out = {k: v.grad.cpu() for k, v in leaves.items()}
        out.update(means2D=means2D.grad.cpu(), radii=radii.cpu())
        out.update({k: v.grad.cpu() for k, v in extra.items()})
        return out
    loss.backward(retain_graph=second_backward)
    first = collect()
    if second_backward:
        for t in list(leaves.values()) + [means2D] + list(extra.values()):
            t.grad = None
        loss.backward()
        first["second"] = collect()
    return first


_runs = {}


def _flagged(name):
    if name not in _runs:
        sc, inp, deg = S.fixture(name)
        _runs[name] = _run(sc, inp, deg, second_backward=True)
    return _runs[name]


@pytest.mark.parametrize("name", list(S.SCENES))
def test_gradient_against_central_differences_of_the_oracle(native_lib, name):
    """1.  dL/d(fx, fy, cx, cy) of the HIP backward against float64 central differences of the oracle, and theta / rho of the same
    backward against the oracle's float64 autograd, all by |got - ref| <= 1e-3 |ref| + 1e-5 max|ref| with no outliers."""
    g = _flagged(name)
    ref = S.central_differences(name)
    ok, worst = S.rel_rule(g["intr"], ref)
    rel = ((g["intr"].double() - ref).abs() / ref.abs()).max().item()
    print(f"{name}: intr {g['intr'].tolist()} ref {ref.tolist()} worst relative error {rel:.2e} ({worst:.3f} of the bound)")
    theta, rho = S.pose_reference(name)
    ok_t, ok_r = S.rel_rule(g["theta"], theta), S.rel_rule(g["rho"], rho)
    print(f"{name}: theta {ok_t[1]:.3f} rho {ok_r[1]:.3f} of the bound")
    assert ok_t[0] and ok_r[0], "the scene sits on a threshold: wrong fixture"
    assert ok, (g["intr"], ref)
    if name == "clamped":
        cx, cy, seen = S.clamp_flags(name)
        assert (cx & seen).sum().item() >= 8 and (cy & seen).sum().item() >= 8
        assert ((g["radii"] > 0) & cx).sum().item() >= 8 and ((g["radii"] > 0) & cy).sum().item() >= 8


@pytest.mark.parametrize("name", ["iso64", "iso257", "aniso2000", "slots70001"])
def test_prepared_and_unprepared_scratch_agree(native_lib, name):
    """2.  The first backward runs on the scratch the forward prepared, a second one through the same forward clears a fresh one with
    a launch: the same four numbers up to the order of the float atomics -- of the blend backward's adds into the gradient lines
    and of the per-workgroup adds into the tau line.  Reordering a float32 sum moves it by a few ulps of the sum of magnitudes; the
    bound is a tenth of the gradient bar (1e-4 |a| + 1e-5 max|a|), far above that and far below a wrong clear (a stale line doubles
    the value)."""
    g = _flagged(name)
    a, b = g["intr"].double(), g["second"]["intr"].double()
    print(f"{name}: prepared {a.tolist()} unprepared {b.tolist()}")
    assert a.abs().min().item() > 0
    assert ((a - b).abs() <= 1e-4 * a.abs() + 1e-5 * a.abs().max()).all()
    for k in ("theta", "rho"):
        a, b = g[k].double(), g["second"][k].double()
        assert ((a - b).abs() <= 1e-4 * a.abs() + 1e-5 * a.abs().max()).all(), k


def test_pose_floats_do_not_depend_on_the_flag_and_default_calls_do_not_change(native_lib):
    """3. and 6.  On the quadrant map (one add per gradient line, one workgroup: nothing depends on an order) the six pose floats are
    bit-identical with and without the flag, and a call without ``intr`` returns bit-identical gradients before any flagged call
    of this test and after one."""
    sc = S.quadrant_scene()
    inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=sc.scales.repeat(1, 3),
               rotations=sc.rotations)
    before = _run(sc, inp, intr=False)
    flagged = _run(sc, inp, intr=True)
    after = _run(sc, inp, intr=False)
    assert (before["radii"] > 0).all() and before["theta"].abs().min().item() > 0 and flagged["intr"].abs().min().item() > 0
    for k in before:
        assert torch.equal(before[k], after[k]), k
        assert torch.equal(before[k], flagged[k]), k          # theta, rho and every other gradient: the flag only adds four sums
    nopose = _run(sc, inp, intr=True, pose=False)             # intr alone asks for the ten-float line as well
    assert torch.equal(nopose["intr"], flagged["intr"])


def test_scene_behind_the_camera_gives_exact_zeros(native_lib):
    """4.  Every Gaussian behind the camera: exactly 0.0 four times (and six times for the pose)."""
    sc, inp, _ = S.fixture("iso257")
    pc = inp["means3D"] @ sc.R.t() + sc.t[None, :]
    pc[:, 2] = -pc[:, 2].abs() - 0.5
    behind = dict(inp, means3D=((pc - sc.t[None, :]) @ sc.R).contiguous())
    g = _run(sc, behind, second_backward=True)
    assert (g["radii"] == 0).all()
    for r in (g, g["second"]):
        assert r["intr"].tolist() == [0.0] * 4 and r["theta"].tolist() == [0.0] * 3 and r["rho"].tolist() == [0.0] * 3


@pytest.mark.parametrize("name", ["aniso65", "iso2000", "clamped", "slots70001"])
def test_principal_point_identity_from_the_backwards_own_outputs(native_lib, name):
    """5.  dL/dcx = sum_i means2D.grad[i, 0] (2 / W) z_i p_w,i and dL/dcy likewise, evaluated in float64 from the means2D.grad the same
    backward returned, within (n + 2) 2^-24 sum|term| (n live Gaussians: the float32 sum of n terms, each formed with two roundings)."""
    sc, inp, deg = S.fixture(name)
    g = _flagged(name)
    st = S.oracle_settings(sc, deg)
    V, PM = st.viewmatrix.double().reshape(-1), st.projmatrix.double().reshape(-1)
    m = inp["means3D"].double()
    z = V[2] * m[:, 0] + V[6] * m[:, 1] + V[10] * m[:, 2] + V[14]
    p_w = 1.0 / ((PM[3] * m[:, 0] + PM[7] * m[:, 1] + PM[11] * m[:, 2] + PM[15]) + 0.0000001)
    live = g["radii"] > 0
    n = int(live.sum())
    W, H = sc.intr["W"], sc.intr["H"]
    for j, (comp, size) in enumerate(((2, W), (3, H))):
        term = (g["means2D"][:, j].double() * (2.0 / size) * z * p_w)[live]
        want, bound = term.sum().item(), (n + 2) * 2.0 ** -24 * term.abs().sum().item()
        got = g["intr"][comp].item()
        print(f"{name}: d/dc{'xy'[j]} {got:.9e} identity {want:.9e} |diff| {abs(got - want):.2e} bound {bound:.2e} (n = {n})")
        assert abs(got - want) <= bound


# ---- the calibration loop ---------------------------------------------------------------------------------------------------------
K160 = dict(fx=133.85, fy=134.8, cx=80.025, cy=61.9, W=160, H=120)
# Measured final |error| / initial |error| on an MI355X (recorded in DESIGN.md section 3); the assertions hold 4 x these, capped
# by the issue's 10 % (all four free, fixed poses) and 50 % (focal + poses).
MEASURED_FIXED = dict(fx=0.0177, fy=0.0008, cx=0.0073, cy=0.0010)      # the same in six runs
MEASURED_FREE = dict(focal=0.0042, pose=0.1207)                        # the worst of six runs (focal 0.0030-0.0042, pose 0.034-0.121)


def _calibration_problem(pose_noise=None):
    from monogs_amd import camera as cam
    from monogs_amd.frames import Intrinsics, Viewpoint
    from monogs_amd.map_step import render_map
    sc = make_scene(2000, K160, seed=21, near_fraction=0.0, device=DEV)
    gmap = SimpleNamespace(get_xyz=sc.means3D, get_rotation=sc.rotations, get_scaling=sc.scales, get_opacity=sc.opacities,
                           get_features=sc.colors, fused_adam=False)
    bg = torch.zeros(3, device=DEV)
    true = Intrinsics(K160, DEV)
    T0 = torch.eye(4, device=DEV)
    T0[:3, :3], T0[:3, 3] = sc.R, sc.t
    views = []
    with torch.no_grad():
        for i, tau in enumerate(([0.0] * 6, [0.15, -0.05, 0.1, 0.02, -0.06, 0.03], [-0.2, 0.1, -0.1, -0.03, 0.05, -0.04])):
            Tm = cam.se3_exp(torch.tensor(tau, device=DEV)) @ T0
            vp = Viewpoint(i, torch.zeros(3, 120, 160, device=DEV), torch.ones(120, 160, device=DEV), DEV)
            vp.update_RT(Tm[:3, :3].contiguous(), Tm[:3, 3].contiguous())
            pkg = render_map(vp, true, gmap, bg)              # the targets: the no-grad forward at the true intrinsics
            v = Viewpoint(i, pkg["render"].clone(), pkg["depth"][0].clone(), DEV, gt_R=Tm[:3, :3].clone(), gt_T=Tm[:3, 3].clone())
            Ts = Tm if pose_noise is None else cam.se3_exp(torch.tensor(pose_noise[i], device=DEV)) @ Tm
            v.update_RT(Ts[:3, :3].contiguous(), Ts[:3, 3].contiguous())
            views.append(v)
    return gmap, views, bg


def _pose_error(views):
    from monogs_amd.frames import position_error
    return max(float(position_error(v)) for v in views)


def test_recovery_of_all_four_against_a_fixed_map(native_lib):
    """7a.  From fx 1.04, fy 0.97, cx + 3, cy - 2 every parameter ends within 10 % of its initial error (the cap) and within four
    times the measured ratio."""
    from monogs_amd.calibration import refine_intrinsics
    from monogs_amd.frames import Intrinsics
    gmap, views, bg = _calibration_problem()
    start = dict(K160, fx=K160["fx"] * 1.04, fy=K160["fy"] * 0.97, cx=K160["cx"] + 3, cy=K160["cy"] - 2)
    intr = Intrinsics(start, DEV, learnable=True)
    traj = refine_intrinsics(gmap, views, intr, bg, iters=80, poses="fixed")
    assert len(traj["k"]) == 81 and len(traj["loss"]) == 80 and traj["loss"][-1] < 0.2 * traj["loss"][0]
    for j, n in enumerate(S.NAMES):
        ratio = abs(traj["k"][-1][j] - K160[n]) / abs(start[n] - K160[n])
        print(f"{n}: start {start[n]:.3f} end {traj['k'][-1][j]:.4f} true {K160[n]:.3f} final / initial error {ratio:.4f}")
        assert ratio <= min(0.10, 4 * MEASURED_FIXED[n]), n
    assert (intr.fx, intr.fy, intr.cx, intr.cy) == tuple(traj["k"][-1]) and intr.delta.abs().max().item() == 0


def test_recovery_of_the_focal_lengths_with_free_poses(native_lib):
    """7b.  ``free=("fx", "fy")``, ``poses="free"`` from poses perturbed by a small tau: the focal error and the pose error both end
    below half their initial values (the cap) and within four times the measured ratios; cx, cy do not move."""
    from monogs_amd.calibration import refine_intrinsics
    from monogs_amd.frames import Intrinsics
    noise = ([0.004, -0.003, 0.002, 0.002, -0.003, 0.001], [-0.003, 0.002, 0.004, -0.002, 0.001, 0.003],
             [0.002, 0.004, -0.003, 0.001, 0.002, -0.002])
    gmap, views, bg = _calibration_problem(pose_noise=noise)
    start = dict(K160, fx=K160["fx"] * 1.04, fy=K160["fy"] * 0.97)
    intr = Intrinsics(start, DEV, learnable=True)
    pose0 = _pose_error(views)
    traj = refine_intrinsics(gmap, views, intr, bg, iters=80, free=("fx", "fy"), poses="free")
    focal = max(abs(traj["k"][-1][j] - K160[n]) / abs(start[n] - K160[n]) for j, n in enumerate(("fx", "fy")))
    pose = _pose_error(views) / pose0
    print(f"focal final / initial error {focal:.4f}; pose error {pose0:.5f} m -> {_pose_error(views):.5f} m ({pose:.4f})")
    assert abs(intr.cx - start["cx"]) < 1e-4 and abs(intr.cy - start["cy"]) < 1e-4       # (float32 copies of the start values)
    assert focal <= min(0.5, 4 * MEASURED_FREE["focal"])
    assert pose <= min(0.5, 4 * MEASURED_FREE["pose"])


def test_step_refuses_stream_capture(native_lib):
    """8.  ``IntrinsicsAdam.step()`` under an active stream capture raises before launching anything: nothing was recorded, the
    parameters and the step counts are untouched."""
    from monogs_amd.calibration import IntrinsicsAdam
    from monogs_amd.frames import Intrinsics
    intr = Intrinsics(K160, DEV, learnable=True)
    opt = IntrinsicsAdam(intr, 0.3, 0.1)
    intr.delta.grad = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    x = torch.zeros(4, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="eager-only"):
            opt.step()
        x.add_(1.0)                                           # (the capture itself is intact: it records and replays this)
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4
    assert opt.t_dev.tolist() == [0, 0] and opt.k.tolist() == [torch.tensor(K160[n]).item() for n in S.NAMES]
    assert (intr.fx, intr.cx) == (K160["fx"], K160["cx"]) and intr.delta.grad is not None
    assert opt.step()[0] < K160["fx"]                          # and the same optimiser steps eagerly
    assert opt.t_dev.tolist() == [1, 1]
