"""The fixture scenes of the intrinsics-gradient tests (tests/test_intrinsics_host.py checks the fixtures themselves without a GPU,
tests/test_gpu_intrinsics.py the HIP backward against them) and their reference: float64 central differences of the oracle's loss
<g_c, colour> + <g_d, depth> in each of fx, fy, cx, cy, with tanfov, projmatrix_raw and projmatrix rebuilt at every step the way
tests/test_oracle.py::test_pose_jacobian_finite_differences rebuilds the pose matrices.

All scenes are 64x48 (the fr3_office intrinsics divided by ten).  The seeds are fixed here: they are the ones for which the
differences at step H_FD and H_FD / 2 agree to 1e-6 relative, i.e. for which no decision of the renderer (radius, rectangle, the
alpha < 1/255 test, termination) flips inside the stencil -- the condition that keeps the reference itself off a threshold."""
import torch

from monogs_amd.camera import ZFAR, ZNEAR
from monogs_amd.synthetic import make_scene, scene_settings
from oracle import OracleSettings, gs_oracle, rasterize, rasterize_autograd

D = torch.float64
K64 = dict(fx=53.54, fy=53.92, cx=32.01, cy=24.76, W=64, H=48)
NAMES = ("fx", "fy", "cx", "cy")
H_FD = 1e-5            # pixels.  The loss is ~1e-2 in float64 (rounding ~1e-18): difference noise ~1e-13 against gradients >= 1e-6

# name -> (kind, P, seed, anisotropic)
SCENES = {}
for _P, _seeds in ((1, (0, 0)), (64, (1, 2)), (65, (3, 4)), (257, (5, 6)), (2000, (7, 9))):
    SCENES[f"iso{_P}"] = ("plain", _P, _seeds[0], False)
    SCENES[f"aniso{_P}"] = ("plain", _P, _seeds[1], True)
SCENES["sh2_257"] = ("sh", 257, 11, True)
SCENES["cov_257"] = ("cov", 257, 12, True)
SCENES["clamped"] = ("clamp", 96, 13, True)
SCENES["slots70001"] = ("slots", 70001, 14, False)


def _clamp_scene(P, seed):
    """Two thirds of the Gaussians sit OUTSIDE 1.3 x the field of view in x or in y (the clamp flag is set) and are large enough for
    their rectangle to reach the image; the rest are an ordinary scene."""
    base = make_scene(P, K64, seed=seed, anisotropic=True, near_fraction=0.0, mean_radius_px=4.0)
    g = torch.Generator().manual_seed(seed + 1000)
    U = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)  # noqa: E731
    n = 2 * P // 3
    tanx, tany = K64["W"] / (2 * K64["fx"]), K64["H"] / (2 * K64["fy"])
    z = 1.0 + 2.0 * U(n)
    side = torch.where(U(n) < 0.5, -1.0, 1.0)
    out = side * (1.34 + 0.2 * U(n))                    # |t / tz| in 1.34 .. 1.54 x tanfov: beyond the 1.3 limit
    inn = 1.6 * U(n) - 0.8
    in_x = torch.arange(n) % 2 == 0                     # alternate: clamped in x, clamped in y
    u, v = torch.where(in_x, out, inn), torch.where(in_x, inn, out)
    pc = torch.stack([u * z * tanx, v * z * tany, z], 1)
    means = base.means3D.clone()
    means[:n] = (pc - base.t[None, :]) @ base.R
    scales = base.scales.clone()
    scales[:n] = (z * (0.10 + 0.08 * U(n)))[:, None] * (0.7 + 0.6 * U(n, 3))      # ~ 8 px sigma: the 3 sigma rectangle reaches in
    return base._replace(means3D=means.contiguous(), scales=scales.contiguous())


def _slots_scene(P, seed):
    """About 2 000 Gaussians in front of the camera, spread evenly over the index range, the rest behind it: more than 256
    workgroups (the tau_part slot path) at the oracle cost of a 2 000-Gaussian scene."""
    n = 2000
    front = make_scene(n, K64, seed=seed, near_fraction=0.0, mean_radius_px=4.0)
    g = torch.Generator().manual_seed(seed + 1000)
    U = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)  # noqa: E731
    pc = torch.stack([4 * U(P) - 2, 4 * U(P) - 2, -(0.5 + 5 * U(P))], 1)      # camera space, z < 0
    means = ((pc - front.t[None, :]) @ front.R).contiguous()
    at = torch.arange(n) * (P // n)
    q = torch.randn(P, 4, generator=g)
    scales, rot = 0.02 + 0.05 * U(P, 1), q / q.norm(dim=1, keepdim=True)
    opac, col = 0.1 + 0.8 * U(P, 1), U(P, 3)
    means[at], scales[at], rot[at], opac[at], col[at] = front.means3D, front.scales, front.rotations, front.opacities, front.colors
    return front._replace(means3D=means, scales=scales.contiguous(), rotations=rot.contiguous(), opacities=opac.contiguous(),
                          colors=col.contiguous())


_cache = {}


def fixture(name):
    """``(scene, inputs, sh_degree)``: ``inputs`` is the oracle's / the rasteriser's keyword dict of float32 CPU tensors."""
    if name in _cache:
        return _cache[name]
    kind, P, seed, aniso = SCENES[name]
    if kind == "clamp":
        sc = _clamp_scene(P, seed)
    elif kind == "slots":
        sc = _slots_scene(P, seed)
    else:
        sc = make_scene(P, K64, seed=seed, anisotropic=aniso, near_fraction=0.0 if P < 100 else 0.01, mean_radius_px=4.0)
    scales = sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)
    inp, deg = dict(means3D=sc.means3D, opacities=sc.opacities), 0
    if kind == "sh":
        g = torch.Generator().manual_seed(seed + 2000)
        sh = 0.3 * torch.randn(P, 9, 3, generator=g)
        sh[:, 0] += 1.0                                   # keeps most colours off the clamp at zero
        inp["shs"], deg = sh, 2
    else:
        inp["colors_precomp"] = sc.colors
    if kind == "cov":
        inp["cov3D_precomp"] = gs_oracle.cov3d_from_scale_rot(scales, sc.rotations, torch.tensor(1.0))
    else:
        inp["scales"], inp["rotations"] = scales, sc.rotations
    _cache[name] = (sc, inp, deg)
    return _cache[name]


def oracle_settings(sc, deg, k=None):
    """The oracle's settings of ``sc``; with ``k = (fx, fy, cx, cy)`` every quantity that depends on the intrinsics is rebuilt in
    float64: tanfov = W / 2 fx, P00 = 2 fx / W, P11 = 2 fy / H, P02 = (2 cx - W) / W, P12 = (2 cy - H) / H, projmatrix = P T_cw."""
    st = scene_settings(sc, OracleSettings, sh_degree=deg)
    if k is None:
        return st
    fx, fy, cx, cy = (float(v) for v in k)
    W, H = sc.intr["W"], sc.intr["H"]
    Pm = torch.zeros(4, 4, dtype=D)
    Pm[0, 0], Pm[1, 1] = 2 * fx / W, 2 * fy / H
    Pm[0, 2], Pm[1, 2] = (2 * cx - W) / W, (2 * cy - H) / H
    Pm[3, 2] = 1.0
    Pm[2, 2], Pm[2, 3] = ZFAR / (ZFAR - ZNEAR), -(ZFAR * ZNEAR) / (ZFAR - ZNEAR)
    T = st.viewmatrix.t().to(D)
    return st._replace(tanfovx=W / (2 * fx), tanfovy=H / (2 * fy), projmatrix_raw=Pm.t().contiguous(),
                       projmatrix=(Pm @ T).t().contiguous(), viewmatrix=st.viewmatrix.to(D), campos=st.campos.to(D))


def k_of(sc):
    return [float(sc.intr[n]) for n in NAMES]


def oracle_loss(name, k):
    sc, inp, deg = fixture(name)
    o = rasterize(inp["means3D"], None, inp["opacities"], oracle_settings(sc, deg, k), shs=inp.get("shs"),
                  colors_precomp=inp.get("colors_precomp"), scales=inp.get("scales"), rotations=inp.get("rotations"),
                  cov3D_precomp=inp.get("cov3D_precomp"), dtype=D)
    return ((o.color * sc.grad_color.to(D)).sum() + (o.depth * sc.grad_depth.to(D)).sum()).item()


_fd = {}


def central_differences(name, h=H_FD):
    """float64 [4]: d loss / d (fx, fy, cx, cy) of the oracle by central differences of step ``h`` pixels (computed once per process)."""
    if (name, h) not in _fd:
        k0 = k_of(fixture(name)[0])
        out = []
        for i in range(4):
            kp, km = list(k0), list(k0)
            kp[i] += h
            km[i] -= h
            out.append((oracle_loss(name, kp) - oracle_loss(name, km)) / (2 * h))
        _fd[(name, h)] = torch.tensor(out, dtype=D)
    return _fd[(name, h)]


_pose = {}


def pose_reference(name):
    """``(theta, rho)`` of the oracle's float64 autograd for the same loss."""
    if name not in _pose:
        sc, inp, deg = fixture(name)
        _, g = rasterize_autograd(inp, oracle_settings(sc, deg), sc.grad_color, sc.grad_depth, dtype=D)
        _pose[name] = (g["theta"], g["rho"])
    return _pose[name]


def clamp_flags(name):
    """bool[P] x 3: (clamp_x, clamp_y, visible) of the oracle's float64 projection."""
    sc, inp, deg = fixture(name)
    st = oracle_settings(sc, deg)
    V = st.viewmatrix.to(D).reshape(-1)
    m = inp["means3D"].to(D)
    pv = [V[k] * m[:, 0] + V[4 + k] * m[:, 1] + V[8 + k] * m[:, 2] + V[12 + k] for k in range(3)]
    cx = (pv[0] / pv[2]).abs() > 1.3 * st.tanfovx
    cy = (pv[1] / pv[2]).abs() > 1.3 * st.tanfovy
    o = rasterize(inp["means3D"], None, inp["opacities"], st, colors_precomp=inp.get("colors_precomp"), shs=inp.get("shs"),
                  scales=inp.get("scales"), rotations=inp.get("rotations"), cov3D_precomp=inp.get("cov3D_precomp"), dtype=D)
    return cx, cy, o.n_touched > 0


def rel_rule(got, ref):
    """The project's elementwise gradient rule (tests/test_gpu_parity.py::_check_grads, north_star's 1e-3) with no outliers allowed:
    ``|got - ref| <= 1e-3 |ref| + 1e-5 max|ref|``.  Returns (ok, worst |got - ref| / that bound)."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    bound = 1e-3 * ref.abs() + 1e-5 * ref.abs().max()
    if ref.abs().max().item() == 0:
        return bool((got == 0).all()), 0.0
    return bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())


def quadrant_scene():
    """A 64x48 map whose rasteriser gradients do not depend on the order of execution: four layers of one Gaussian per 8 x 8 quadrant,
    each well inside its quadrant (screen variance 0.6 + 0.3: alpha is below 1/255 at the quadrant's border), so every gradient line
    receives ONE add of the blend backward; P = 192 is one workgroup of the per-Gaussian backward, so the tau line has no order either.
    Identity pose (the construction of tests/test_gpu_object_motion.py::_quadrant_scene)."""
    k = K64
    g = torch.Generator().manual_seed(4)
    qx, qy = torch.meshgrid(torch.arange(8.0), torch.arange(6.0), indexing="ij")
    px, py = (8 * qx + 3.5).reshape(-1).repeat(4), (8 * qy + 3.5).reshape(-1).repeat(4)
    z = torch.cat([torch.full((48,), 2.0 + 0.1 * layer) for layer in range(4)])
    xyz = torch.stack([(px + 0.5 - k["cx"]) * z / k["fx"], (py + 0.5 - k["cy"]) * z / k["fy"], z], 1)
    P = xyz.shape[0]
    sc = make_scene(P, K64, seed=4, pose_tau=(0.0,) * 6)
    return sc._replace(means3D=xyz.contiguous(), scales=((0.6 ** 0.5) * z / k["fx"])[:, None].contiguous(),
                       rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1), opacities=torch.full((P, 1), 0.7),
                       colors=0.2 + 0.6 * torch.rand(P, 3, generator=g))
