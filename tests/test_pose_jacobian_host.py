"""Pose-tangent rendering without a GPU: the float64 mirror the GPU tests compare against (tests/pose_jacobian_mirror.py) is itself
checked -- its adjoint identity against the oracle's autograd, and against central differences of the oracle's images with the
camera moved and every matrix rebuilt --, and the C ABI's new entry points refuse bad arguments before they launch anything."""
import ctypes
import os
import re

import pytest
import torch

import intrinsics_scenes as S
import pose_jacobian_mirror as M
from oracle import gs_oracle, rasterize, rasterize_autograd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


@pytest.mark.parametrize("name", ["iso64", "aniso257", "clamped"])
def test_mirror_satisfies_the_adjoint_identity(name):
    """sum over p and c < 4 of g[c, p] J[k, c, p] = dL/dtau_k of the oracle's autograd for the scene's cotangent images."""
    sc, inp, deg = S.fixture(name)
    st = S.oracle_settings(sc, deg)
    J, _ = M.oracle_jacobian(inp, st)
    _, g = rasterize_autograd(inp, st, sc.grad_color, sc.grad_depth, dtype=D)
    ref = torch.cat([g["rho"], g["theta"]])
    cot = torch.cat([sc.grad_color.to(D), sc.grad_depth.to(D)], dim=0)
    got = (J[:, :4] * cot[None]).sum(dim=(1, 2, 3))
    print(name, (got - ref).abs().max().item(), ref.abs().max().item())
    assert ref.abs().min().item() > 0
    assert ((got - ref).abs() <= 2e-12 * ref.abs().max()).all(), (got, ref)
    assert J[:, 4].abs().max().item() > 0          # the opacity planes are not part of the identity: at least not empty


def test_mirror_against_central_differences():
    """Every plane against central differences of the oracle's images with T_cw <- exp(tau^) T_cw and the matrices rebuilt, on a
    scene without clamped Gaussians and without capped alphas (the two places where the convention is not the derivative)."""
    sc, inp, deg = S.fixture("iso64")
    # (every matrix rebuilt in float64 from the pose: the float32 product in the plain settings is 1e-7 off P T_cw, which moves the
    #  base point of the derivative, not of the differences below)
    st = S.oracle_settings(sc, deg, S.k_of(sc))
    cx, cy, seen = S.clamp_flags("iso64")
    assert not (cx & seen).any() and not (cy & seen).any() and inp["opacities"].max().item() < 0.99
    J, _ = M.oracle_jacobian(inp, st)
    T0, P = st.viewmatrix.t().to(D), st.projmatrix_raw.t().to(D)

    def images(tau):
        Tn = gs_oracle.se3_exp(tau) @ T0
        st2 = st._replace(viewmatrix=Tn.t().contiguous(), projmatrix=(P @ Tn).t().contiguous(), campos=-(Tn[:3, :3].t() @ Tn[:3, 3]))
        o = rasterize(inp["means3D"], None, inp["opacities"], st2, colors_precomp=inp["colors_precomp"], scales=inp["scales"],
                      rotations=inp["rotations"], dtype=D)
        return torch.cat([o.color, o.depth, o.opacity], dim=0)
    h = 1e-6
    for k in range(6):
        e = torch.zeros(6, dtype=D)
        e[k] = h
        fd = (images(e) - images(-e)) / (2 * h)
        for c in range(5):
            err = (J[k, c] - fd[c]).abs().max().item()
            assert err <= 1e-6 * J[k, c].abs().max().item() + 1e-9, (k, c, err, J[k, c].abs().max().item())


def test_header_and_binding_agree_on_abi_29_and_the_new_symbols(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 29
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    assert re.search(r"#define MGS_GN_SYSTEM_DOUBLES 75\b", text) and re.search(r"#define MGS_GN_FIX_EXPOSURE 2\b", text)
    for s in ("mgs_pose_tangent_bytes", "mgs_pose_jacobian", "mgs_gn_scratch_bytes", "mgs_gn_normal_equations", "mgs_pose_gn_step"):
        assert s in _lib.SIGNATURES and hasattr(native_lib, s), s


def test_scratch_sizes(native_lib):
    assert native_lib.mgs_pose_tangent_bytes(0) == native_lib.mgs_pose_tangent_bytes(-5) > 0
    assert native_lib.mgs_pose_tangent_bytes(1000) - native_lib.mgs_pose_tangent_bytes(0) == 1000 * 192
    assert native_lib.mgs_gn_scratch_bytes(0, 10) == 0 and native_lib.mgs_gn_scratch_bytes(1, 1) == 75 * 8
    assert native_lib.mgs_gn_scratch_bytes(640, 480) == 256 * 75 * 8


def _cam(native_lib, sh_coeffs=0):
    from monogs_amd import _lib
    cam = _lib.MgsCamera()
    cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, cam.scale_modifier = 16, 16, 0.5, 0.5, 1.0
    cam.sh_coeffs, cam.scale_dim = sh_coeffs, 3
    for f in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos"):
        setattr(cam, f, 0x1000)                      # non-NULL and never dereferenced: every check comes before a launch
    return cam


def test_pose_jacobian_argument_errors_return_before_a_launch(native_lib):
    p = 0x1000
    good = dict(P=4, R=8, means3D=p, scales=p, rotations=p, cov=None, radii=p, geometry=p, binning=p, image=p, scratch=p, J=p)

    def call(cam, **kw):
        a = dict(good, **kw)
        return native_lib.mgs_pose_jacobian(ctypes.byref(cam) if cam is not None else None, a["P"], a["R"], a["means3D"], a["scales"],
                                            a["rotations"], a["cov"], a["radii"], a["geometry"], a["binning"], a["image"],
                                            a["scratch"], a["J"], None)
    cam = _cam(native_lib)
    assert call(None) == 1
    assert call(cam, P=-1) == 1
    assert call(cam, P=1 << 26) == 1 and b"MGS_MAX_GAUSSIANS" in native_lib.mgs_last_error()
    assert call(_cam(native_lib, sh_coeffs=9)) == 1 and b"colors_precomp" in native_lib.mgs_last_error()
    for k in ("means3D", "radii", "geometry", "image", "scratch", "J", "binning"):
        assert call(cam, **{k: None}) == 1, k
    assert call(cam, scales=None) == 1 and call(cam, rotations=None) == 1          # half a pair
    assert call(cam, cov=p) == 1                                                    # both forms
    assert call(cam, scales=None, rotations=None) == 1                              # neither
    nocam = _cam(native_lib)
    nocam.viewmatrix = None
    assert call(nocam) == 1
    nocam = _cam(native_lib)
    nocam.image_width = 0
    assert call(nocam) == 1


def test_gauss_newton_argument_errors_return_before_a_launch(native_lib):
    p = 0x1000
    ne = native_lib.mgs_gn_normal_equations
    good = [16, 16, 1, p, p, p, p, p, p, None, p, p, p, 0.05, 0.05, p, p, None]

    def with_(i, v):
        a = list(good)
        a[i] = v
        return ne(*a)
    assert with_(0, 0) == 1 and with_(1, -1) == 1 and with_(2, 2) == 1              # size, MGS_LOSS_INVERT_DEPTH is not a mode here
    for i in (3, 4, 6, 7, 10, 15, 16):                                               # J, render, opacity, gt_rgb, grad_mask, scratch, system
        assert with_(i, None) == 1, i
    assert with_(5, None) == 1 and with_(8, None) == 1                               # depth, gt_depth without MGS_LOSS_RGB_ONLY
    assert with_(11, None) == 1                                                      # half an exposure pair
    assert with_(13, 0.0) == 1 and with_(14, -1.0) == 1
    assert with_(16, p + 4) == 1                                                     # misaligned system
    st = native_lib.mgs_pose_gn_step
    good = [p, p, p, p, p, 1e-3, 0.0, 0.05, 0.05, 1e-4, p, 0, None, None, None, None, None, None]

    def step_(i, v):
        a = list(good)
        a[i] = v
        return st(*a)
    for i in (0, 1, 4, 10):
        assert step_(i, None) == 1, i
    assert step_(2, None) == 1                                                       # half an exposure pair
    assert step_(5, -1.0) == 1 and step_(7, 0.0) == 1 and step_(8, 0.0) == 1
    assert step_(11, 4) == 1                                                         # unknown flag
    assert step_(14, p) == 1                                                         # a partial camera refresh
