"""Surface depth without a GPU: the ABI (v31), the refusals of ``mgs_surface_depth`` / ``mgs_depth_normals``, the CPU mirror of the
specification (tests/surface_mirror.py) tied to the oracle, and the conditions the test scenes must keep meeting -- so that what
tests/test_gpu_surface.py holds the kernels to is itself held to something."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import surface_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")
H, W = M.INTR["H"], M.INTR["W"]
NAN = float("nan")


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_v31(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 31
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    assert _lib.H.MGS_SURFACE_MEDIAN == 1 and _lib.H.MGS_SURFACE_VARIANCE == 2
    for name in ("mgs_surface_depth", "mgs_depth_normals"):
        assert name in _lib.SIGNATURES and hasattr(native_lib, name)
    from monogs_amd import surface
    import monogs_amd
    for name in ("surface_depth", "depth_normals", "eval_geometry"):
        assert getattr(monogs_amd, name) is getattr(surface, name)


def test_surface_unit_is_built_and_included_by_nothing():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bsurface\.hip\b", mk, flags=re.M)
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h")):
            assert not re.search(r'#\s*include\s*"surface\.', open(os.path.join(CSRC, f)).read()), f
    text = open(os.path.join(CSRC, "surface.hip")).read()
    for h in ("common.h", "feat_walk.h", "tile_walk.h"):
        assert f'#include "{h}"' in text


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _cam():
    from monogs_amd import _lib
    cam = _lib.MgsCamera()
    cam.image_height, cam.image_width = 16, 16
    for f in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos"):
        setattr(cam, f, 0x1000)                      # non-NULL and never dereferenced: the checks come first
    return cam


def test_surface_depth_refuses_bad_arguments(native_lib):
    """Every refusal returns 1 with a message before anything is launched (no GPU needed)."""
    cam = _cam()
    X = 0x1000                                       # a non-NULL plane or scratch pointer, never dereferenced
    MED, VAR = 1, 2

    def call(P=8, want=MED | VAR, min_opacity=0.0, max_std=0.0, median=X, mid=None, var=X, scratch=(X, X, X), cam_=cam):
        return native_lib.mgs_surface_depth(ctypes.byref(cam_) if cam_ is not None else None, P, 1, *scratch, want, min_opacity,
                                            max_std, median, mid, var, None)

    cases = [(dict(want=0), b"want"), (dict(want=4), b"want"), (dict(want=7), b"want"), (dict(want=-1), b"want"),
             (dict(median=None), b"median_depth"), (dict(want=MED, median=None), b"median_depth"),
             (dict(var=None), b"depth_var"), (dict(want=VAR, var=None), b"depth_var"),
             (dict(min_opacity=NAN), b"min_opacity"), (dict(min_opacity=-0.1), b"min_opacity"),
             (dict(max_std=NAN), b"max_std"), (dict(max_std=-1.0), b"max_std"),
             (dict(want=MED, max_std=0.05), b"MGS_SURFACE_VARIANCE"), (dict(want=MED, max_std=0.05, var=None), b"MGS_SURFACE_VARIANCE"),
             (dict(P=-1), b"P must be"), (dict(P=1 << 26), b"MGS_MAX_GAUSSIANS"),
             (dict(scratch=(None, X, X)), b"geometry"), (dict(scratch=(X, X, None)), b"image"), (dict(scratch=(X, None, X)), b"binning")]
    for kw, word in cases:
        assert call(**kw) == 1, kw
        assert word in native_lib.mgs_last_error(), (kw, native_lib.mgs_last_error())
    assert call(cam_=None) == 1
    bad = _cam()
    bad.image_width = 0                              # non-positive sizes
    assert call(cam_=bad) == 1
    bad.image_width, bad.image_height = 16, -3
    assert call(cam_=bad) == 1


def test_depth_normals_refuses_bad_arguments(native_lib):
    X = 0x1000

    def call(W_=16, H_=16, depth=X, fx=80.0, fy=80.0, cx=8.0, cy=8.0, max_jump=0.0, out=X):
        return native_lib.mgs_depth_normals(W_, H_, depth, fx, fy, cx, cy, max_jump, out, None)

    for kw, word in [(dict(W_=0), b"positive"), (dict(H_=-2), b"positive"), (dict(W_=1 << 16, H_=1 << 15), b"2^31"),
                     (dict(depth=None), b"depth"), (dict(out=None), b"normals"), (dict(fx=0.0), b"fx"), (dict(fy=NAN), b"fx"),
                     (dict(fy=-3.0), b"fx"), (dict(cx=NAN), b"cx"), (dict(max_jump=NAN), b"max_jump"), (dict(max_jump=-0.5), b"max_jump")]:
        assert call(**kw) == 1, kw
        assert word in native_lib.mgs_last_error(), (kw, native_lib.mgs_last_error())


def test_python_layer_refuses_before_the_library():
    from monogs_amd.surface import depth_normals, surface_depth
    color = torch.zeros(3, 4, 4)
    with pytest.raises(ValueError, match="want must hold"):
        surface_depth(color, want=("mean",))
    with pytest.raises(ValueError, match="empty"):
        surface_depth(color, want=())
    with pytest.raises(ValueError, match="variance"):
        surface_depth(color, want=("median",), max_std=0.1)
    with pytest.raises(ValueError, match="want_id"):
        surface_depth(color, want=("variance",), want_id=True)
    with pytest.raises(RuntimeError, match="surface_depth needs the colour image of a differentiable rasteriser forward"):
        surface_depth(color)
    with pytest.raises(RuntimeError, match="no CPU path"):
        depth_normals(torch.ones(4, 4), None)


def test_fuse_map_refuses_unknown_depth_modes():
    from monogs_amd.tsdf import fuse_map

    class OneGaussian:
        def __len__(self):
            return 1
    with pytest.raises(ValueError, match="mean.*median"):
        fuse_map(OneGaussian(), [], None, None, None, depth="mode")
    with pytest.raises(ValueError, match="max_std"):
        fuse_map(OneGaussian(), [], None, None, None, depth="mean", max_std=0.05)


# ---- the mirror, tied to the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi", "veil", "sparse", "stack"])
def test_mirror_sums_reproduce_the_oracle_depth_in_float64(name):
    """z_1 O + S1 = sum w z: with every quantity in float64 the mirror's walk gives the oracle's depth image to 1e-12."""
    o = M.oracle(name, torch.float64)
    m = M.surface_mirror(o.aux, H, W, sum_dtype=torch.float64)
    assert m.O.dtype == torch.float64 and o.depth.dtype == torch.float64
    err = (m.z1 * m.O + m.S1 - o.depth[0]).abs().max().item()
    print(f"{name}: max |z1 O + S1 - depth| = {err:.2e}")
    assert err <= 1e-12
    assert ((m.O - o.opacity[0]).abs().max().item()) <= 1e-12
    assert (m.depth_var >= 0).all() and (m.depth_var[m.O == 0] == 0).all()


@pytest.mark.parametrize("name", list(M.SCENES))
def test_mirror_median_agrees_with_the_oracle(name):
    o = M.oracle(name)
    m = M.surface_mirror(o.aux, H, W)
    amb = o.aux["ambiguous"]
    has = m.median_pos > 0
    # a median exists exactly when the final transmittance is <= 0.5
    assert torch.equal(has[~amb], (o.aux["final_T"][0] <= 0.5)[~amb])
    # the contributors in front of the median are the ones the forward counted in n_touched
    assert torch.equal(m.before_median.to(torch.int32), o.n_touched)
    assert torch.equal(m.median_id >= 0, has) and torch.equal(m.median_depth != 0, has)
    assert torch.equal(m.median_depth[has], o.aux["geom"]["depth"][m.median_id[has]])
    assert m.median_depth.dtype == torch.float32
    assert (m.median_pos <= o.aux["n_contrib"][0]).all()


def test_stack_closed_form():
    """Opacities 0.3 / 0.4 / 0.9 at depths 1 / 2 / 3 over the centre: t = 0.7, 0.42 -- the median is the second; the variance is that
    of the three depths under the weights 0.3, 0.28, 0.378."""
    o = M.oracle("stack")
    m = M.surface_mirror(o.aux, H, W)
    x0, y0 = (int(round(float(v))) for v in o.aux["geom"]["xy"][0])
    ys, xs = slice(y0 - 1, y0 + 2), slice(x0 - 1, x0 + 2)
    assert (m.median_pos[ys, xs] == 2).all() and (m.median_id[ys, xs] == 1).all()
    assert (m.median_depth[ys, xs] == o.aux["geom"]["depth"][1]).all() and abs(float(o.aux["geom"]["depth"][1]) - 2.0) < 1e-5
    w = np.array([0.3, 0.7 * 0.4, 0.42 * 0.9])
    z = np.array([1.0, 2.0, 3.0])
    mean = (w * z).sum() / w.sum()
    var = (w * (z - mean) ** 2).sum() / w.sum()
    assert (m.depth_var[ys, xs] - var).abs().max().item() < 5e-3          # (the falloff a pixel off the centre: alpha a little below)
    g = M.surface_mirror(o.aux, H, W, min_opacity=0.9, max_std=0.5)       # opacity 0.958; std 0.83 > 0.5: the spread gate clears it
    assert (g.median_id[ys, xs] == -1).all() and (g.median_depth[ys, xs] == 0).all() and not g.opacity_gate[ys, xs].any()


# ---- scene conditions: nobody weakens a scene unnoticed --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.SCENES))
def test_scenes_stay_within_the_ambiguous_cap(name):
    amb = M.oracle(name).aux["ambiguous"]
    share = amb.float().mean().item()
    print(f"{name}: {int(amb.sum())} ambiguous pixels of {amb.numel()}")
    assert share < 1e-3


def test_scene_conditions():
    pos = {n: M.surface_mirror(M.oracle(n).aux, H, W).median_pos for n in ("multi", "veil", "haze", "long", "sparse")}
    count = lambda n, f: int(f(pos[n]).sum())  # noqa: E731
    for n in pos:
        print(n, "no median", count(n, lambda p: p == 0), "beyond 64", count(n, lambda p: p > 64), "beyond 128",
              count(n, lambda p: p > 128), "deepest", int(pos[n].max()))
    assert count("multi", lambda p: p == 0) == 0 and int(pos["multi"].max()) <= 64          # the early leave after the first step
    assert count("veil", lambda p: p == 0) >= 1000 and count("veil", lambda p: p > 64) >= 2000 and count("veil", lambda p: p > 128) >= 500
    assert count("haze", lambda p: p == 0) >= 5000
    assert count("long", lambda p: p == 0) == 0
    length = lambda n: M.oracle(n).aux["ranges"][:, 1] - M.oracle(n).aux["ranges"][:, 0]  # noqa: E731
    assert int(length("long").max()) > 1024                                                 # lists far longer than the median's position
    assert (M.oracle("sparse").opacity[0] == 0).float().mean().item() > 0.7                 # pixels without a contributor ...
    assert int((length("sparse") == 0).sum()) > 0                                           # ... and empty tiles


# ---- the normals mirror -----------------------------------------------------------------------------------------------------
def _plane_depth(n, c, intr, Hh, Ww):
    """The depth image of the plane n . X = c: d = c / (n . ray), ray = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)."""
    xs, ys = np.meshgrid(np.arange(Ww, dtype=np.float64), np.arange(Hh, dtype=np.float64))
    rx, ry = (xs + 0.5 - intr["cx"]) / intr["fx"], (ys + 0.5 - intr["cy"]) / intr["fy"]
    return c / (n[0] * rx + n[1] * ry + n[2])


def test_depth_normals_mirror_on_a_tilted_plane():
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    d = _plane_depth(n, -2.0, M.INTR, H, W)                    # n . X = -2 with n_z < 0: in front of the camera, facing it
    assert (d > 0).all()
    out = M.depth_normals(d, M.INTR["fx"], M.INTR["fy"], M.INTR["cx"], M.INTR["cy"])
    assert out.shape == (3, H, W)
    assert np.abs(out[:, 1:-1, 1:-1] - n[:, None, None]).max() < 1e-9
    for border in (out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1]):
        assert (border == 0).all()
    # a hole zeroes itself and its four neighbours, nothing else
    h = d.copy()
    h[20, 30] = 0.0
    h[40, 50] = -1.0
    oh = M.depth_normals(h, M.INTR["fx"], M.INTR["fy"], M.INTR["cx"], M.INTR["cy"])
    zero = (oh == 0).all(0)
    expect = np.zeros((H, W), bool)
    expect[0], expect[-1], expect[:, 0], expect[:, -1] = True, True, True, True
    for y, x in ((20, 30), (40, 50)):
        for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
            expect[y + dy, x + dx] = True
    assert (zero == expect).all()
    # a step larger than max_jump zeroes the pixels on both sides of it; without the gate they have normals
    s = d.copy()
    s[:, 60:] += 0.5
    gated = (M.depth_normals(s, M.INTR["fx"], M.INTR["fy"], M.INTR["cx"], M.INTR["cy"], max_jump=0.2) == 0).all(0)
    free = (M.depth_normals(s, M.INTR["fx"], M.INTR["fy"], M.INTR["cx"], M.INTR["cy"]) == 0).all(0)
    assert gated[1:-1, 59:61].all() and not gated[1:-1, 1:59].any() and not gated[1:-1, 61:-1].any()
    assert not free[1:-1, 1:-1].any()
    # float32: the same image to float32 rounding
    o32 = M.depth_normals(d.astype(np.float32), M.INTR["fx"], M.INTR["fy"], M.INTR["cx"], M.INTR["cy"], dtype=np.float32)
    assert o32.dtype == np.float32 and np.abs(o32 - out).max() < 1e-3
    assert math.isclose(float(np.linalg.norm(out[:, 30, 30])), 1.0, rel_tol=1e-12)
