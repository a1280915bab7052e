"""K-channel feature rendering (csrc/features.hip, monogs_amd/feature_render.py) against the CPU oracle and against the
rasteriser's own forward (run on the MI355X box: pytest -m gpu).

The reference for the blend is the oracle called ceil(K / 3) times with ``colors_precomp`` = a zero-padded triple of feature
columns and ``bg = 0``: blending is linear and independent per channel, so that is exact.

Bars (those of tests/test_gpu_parity.py): pixel Linf <= 1e-4 on the pixels the oracle does not flag ambiguous (a decision within
a few ulps of its threshold), the ambiguous share < 1e-3; gradients relative L2 <= 1e-4 and elementwise
|got - ref| <= 1e-3 |ref| + 1e-5 max|ref| for all but a 2e-4 share of the elements.

All scenes render at 104 x 72: 7 x 5 tiles with a half tile on both far edges.
  multi   lists of 98-252 instances (2-4 steps), 27 % of the pixels stop before their list ends
  long    lists up to 1849 (> TDS_CAP: the long-list branch of the per-tile sort), every pixel saturated
  sparse  23 of 35 tiles empty, 5904 pixels without a contributor
"""
import functools
import math

import pytest
import torch

from monogs_amd.debug import options
from monogs_amd.synthetic import make_scene, scene_settings
from oracle import OracleSettings, rasterize, rasterize_autograd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INTR = dict(fx=87.0, fy=87.6, cx=52.0, cy=37.1, W=104, H=72)
H, W = INTR["H"], INTR["W"]
SCENES = dict(multi=lambda: make_scene(3000, INTR, seed=3),
              long=lambda: make_scene(12000, INTR, seed=8, mean_radius_px=12.0),
              sparse=lambda: make_scene(120, INTR, seed=6, mean_radius_px=4.0, spread=0.45))


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


def _features(P, K, seed=0):
    return torch.rand(P, K, generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float32)


def _scales(sc):
    return sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)


def _triples(feat):
    """The feature columns as zero-padded [P,3] colour triples."""
    P, K = feat.shape
    pad = torch.zeros(P, 3 * math.ceil(K / 3))
    pad[:, :K] = feat
    return [pad[:, 3 * i:3 * i + 3].contiguous() for i in range(pad.shape[1] // 3)]


@functools.lru_cache(maxsize=None)
def _oracle_forward(name, K):
    """(feature image [K,H,W], ambiguous [H,W], opacity [H,W]) of the oracle; computed once per (scene, K), never modified."""
    sc = _scene(name)
    st = scene_settings(sc, OracleSettings)           # the scenes' bg is 0
    outs = [rasterize(sc.means3D, None, sc.opacities, st, colors_precomp=c, scales=_scales(sc), rotations=sc.rotations,
                      want_ambiguous=True) for c in _triples(_features(sc.means3D.shape[0], K))]
    amb = torch.stack([o.aux["ambiguous"] for o in outs]).any(0)
    return torch.cat([o.color for o in outs])[:K], amb, outs[0].opacity[0]


def _grad_out(K, seed=0):
    g = torch.Generator().manual_seed(500 + seed)
    return (2 * torch.rand(K, H, W, generator=g) - 1) / (H * W)


@functools.lru_cache(maxsize=None)
def _oracle_backward(name, K):
    """dL/dfeatures [P,K] of the oracle: its colour gradient per triple, grad_depth = 0."""
    sc = _scene(name)
    st = scene_settings(sc, OracleSettings)
    P = sc.means3D.shape[0]
    g = _grad_out(K)
    gpad = torch.zeros(3 * math.ceil(K / 3), H, W)
    gpad[:K] = g
    cols = []
    for i, c in enumerate(_triples(_features(P, K))):
        inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=c, scales=_scales(sc), rotations=sc.rotations)
        _, og = rasterize_autograd(inp, st, gpad[3 * i:3 * i + 3], torch.zeros(1, H, W), dtype=torch.float32)
        cols.append(og["colors_precomp"])
    return torch.cat(cols, 1)[:, :K]


def _forward(sc, colors=None, grad=True, bg3=None):
    """A rasteriser forward of the scene; returns (color, radii, depth, opacity, leaves)."""
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    if bg3 is not None:
        sc = sc._replace(bg=torch.tensor(bg3, dtype=torch.float32))
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(grad)  # noqa: E731
    leaves = dict(means3D=leaf(sc.means3D), opacities=leaf(sc.opacities),
                  colors_precomp=leaf(sc.colors if colors is None else colors), scales=leaf(_scales(sc)),
                  rotations=leaf(sc.rotations))
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=grad)
    leaves["theta"] = torch.zeros(3, device=DEV, requires_grad=grad)
    leaves["rho"] = torch.zeros(3, device=DEV, requires_grad=grad)
    color, radii, depth, opacity, n_touched = GaussianRasterizer(st)(**leaves)
    return color, radii, depth, opacity, leaves


def _check_pixels(got, ref, amb, what, scale=1.0):
    err = (got - ref).abs()
    err = err.amax(0) if err.dim() == 3 else err
    share = amb.float().mean().item()
    print(f"{what}: ambiguous share {share:.1e}; Linf clear {err[~amb].max():.2e}, Linf all {err.max():.2e}")
    assert share < 1e-3
    assert err[~amb].max() <= 1e-4 * scale, what


def _check_grad(got, ref, what, rtol=1e-3, max_outlier_frac=2e-4, l2_tol=1e-4):
    got, ref = got.double().cpu(), ref.double()
    scale = ref.abs().max().item()
    if scale == 0:
        assert got.abs().max().item() == 0, what
        return
    rel_l2 = ((got - ref).norm() / ref.norm()).item()
    bad = ((got - ref).abs() > rtol * ref.abs() + 1e-5 * scale).float().mean().item()
    print(f"{what}: relative L2 {rel_l2:.2e}, outliers {bad:.1e}")
    assert rel_l2 <= l2_tol, what
    assert bad <= max_outlier_frac, what


# ---- 1. forward against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("multi", 1), ("multi", 5), ("multi", 16), ("multi", 33), ("long", 16), ("sparse", 1),
                                    ("sparse", 5)])
def test_forward_vs_oracle(native_lib, name, K):
    from monogs_amd import render_features
    sc = _scene(name)
    ref, amb, opac = _oracle_forward(name, K)
    feat = _features(sc.means3D.shape[0], K).to(DEV)
    color, *_ = _forward(sc)
    out = render_features(color, feat)
    assert out.shape == (K, H, W) and out.dtype == torch.float32
    _check_pixels(out.cpu(), ref, amb, f"{name} K={K}")
    if name == "sparse":
        empty = opac == 0                                  # pixels without a contributor (oracle)
        assert int(empty.sum()) == 5904
        assert (out.cpu()[:, empty] == 0).all()
        bg = torch.linspace(0.1, 0.9, K, device=DEV)
        out_bg = render_features(color, feat, bg=bg).cpu()
        assert (out_bg[:, empty] == bg.cpu()[:, None]).all()


# ---- 2. forward against the project's own forward -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi", "long"])
def test_forward_reproduces_colour_depth_opacity(native_lib, name):
    from monogs_amd import render_features
    from monogs_amd.debug import forward_tables
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    sc = _scene(name)
    _, amb, _ = _oracle_forward(name, 16 if name == "long" else 5)
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    t = forward_tables(st, sc.means3D.to(DEV), sc.opacities.to(DEV), colors_precomp=sc.colors.to(DEV),
                       scales=_scales(sc).to(DEV), rotations=sc.rotations.to(DEV))
    z = t["rec"][:, 11].clone()                            # the record's depth (garbage for culled Gaussians: in no list)
    z[t["radii"] == 0] = 0
    feat = torch.cat([sc.colors.to(DEV), z[:, None], torch.ones_like(z)[:, None]], 1).contiguous()
    color, radii, depth, opacity, _ = _forward(sc)
    out = render_features(color, feat, bg=torch.zeros(5, device=DEV)).cpu()
    _check_pixels(out[0:3], color.detach().cpu(), amb, f"{name} colour")
    _check_pixels(out[3], depth.detach().cpu()[0], amb, f"{name} depth", scale=max(1.0, depth.max().item()))
    _check_pixels(out[4], opacity.detach().cpu()[0], amb, f"{name} opacity")


# ---- 3. background ------------------------------------------------------------------------------------------------------
def test_background_term(native_lib):
    from monogs_amd import render_features
    from monogs_amd.debug import forward_tables
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    sc = _scene("multi")
    feat = _features(sc.means3D.shape[0], 5).to(DEV)
    bg = torch.tensor([0.9, 0.1, 0.5, 0.3, 0.7], device=DEV)
    color, _, _, opacity, _ = _forward(sc)
    final_T = forward_tables(scene_settings(sc, GaussianRasterizationSettings, device=DEV), sc.means3D.to(DEV),
                             sc.opacities.to(DEV), colors_precomp=sc.colors.to(DEV), scales=_scales(sc).to(DEV),
                             rotations=sc.rotations.to(DEV))["final_T"]
    assert torch.equal(1.0 - final_T, opacity.detach()[0])
    d = render_features(color, feat, bg=bg) - render_features(color, feat)
    assert (d - final_T[None] * bg[:, None, None]).abs().max() <= 1e-6


# ---- 4. labels: exact, no exemptions ------------------------------------------------------------------------------------
def _lowest_argmax(img):
    K = img.shape[0]
    idx = torch.arange(K, device=img.device)[:, None, None].expand_as(img)
    return torch.where(img == img.amax(0, keepdim=True), idx, K).amin(0)


@pytest.mark.parametrize("name,K,min_opacity", [("multi", 7, 0.5), ("sparse", 7, 0.5), ("multi", 40, 0.5), ("sparse", 7, 0.0),
                                                ("multi", 40, 0.0)])
def test_labels(native_lib, name, K, min_opacity):
    from monogs_amd import render_features
    sc = _scene(name)
    P = sc.means3D.shape[0]
    ids = torch.randint(0, K, (P,), generator=torch.Generator().manual_seed(7))
    feat = torch.nn.functional.one_hot(ids, K).float().to(DEV)
    color, _, _, opacity, _ = _forward(sc)
    out, labels = render_features(color, feat, want_labels=True, min_opacity=min_opacity)
    assert labels.shape == (H, W) and labels.dtype == torch.int32
    opaque = opacity.detach()[0] >= min_opacity
    assert torch.equal(labels == -1, ~opaque)
    assert torch.equal(labels[opaque].long(), _lowest_argmax(out.detach())[opaque])
    if min_opacity == 0.0:
        assert (labels >= 0).all()
    elif name == "sparse":
        assert (labels == -1).any() and (labels >= 0).any()


# ---- 5. backward against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("multi", 5), ("long", 16), ("sparse", 1), ("multi", 33)])
def test_backward_vs_oracle(native_lib, name, K):
    from monogs_amd import render_features
    sc = _scene(name)
    ref = _oracle_backward(name, K)
    feat = _features(sc.means3D.shape[0], K).to(DEV).requires_grad_(True)
    color, radii, *_ = _forward(sc)
    out = render_features(color, feat)
    g = _grad_out(K).to(DEV)
    (g1,) = torch.autograd.grad(out, feat, g, retain_graph=True)
    _check_grad(g1, ref, f"{name} K={K}")
    assert (g1[radii == 0] == 0).all() and bool((radii == 0).any())
    (g2,) = torch.autograd.grad(out, feat, g)             # the call clears its own output: nothing accumulates
    _check_grad(g2, ref, f"{name} K={K}, second backward")


# ---- 6. beside the rasteriser's backward --------------------------------------------------------------------------------
def test_beside_the_rasteriser_backward(native_lib):
    from monogs_amd import render_features
    sc = _scene("multi")
    K = 5
    ref_feat = _oracle_backward("multi", K)
    inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=_scales(sc), rotations=sc.rotations)
    _, ograds = rasterize_autograd(inp, scene_settings(sc, OracleSettings), sc.grad_color, sc.grad_depth, dtype=torch.float32)
    feat = _features(sc.means3D.shape[0], K).to(DEV).requires_grad_(True)
    color, radii, depth, opacity, leaves = _forward(sc)
    out = render_features(color, feat)
    g = _grad_out(K).to(DEV)
    loss = (color * sc.grad_color.to(DEV)).sum() + (depth * sc.grad_depth.to(DEV)).sum() + (out * g).sum()
    loss.backward()
    for k, ref in ograds.items():
        _check_grad(leaves[k].grad.reshape(ref.shape), ref, f"rasteriser {k}")
    _check_grad(feat.grad, ref_feat, "features beside the rasteriser")
    # the rasteriser's graph is freed now; the feature render kept its own references to the tables
    feat.grad = None
    (render_features(color, feat) * g).sum().backward()
    _check_grad(feat.grad, ref_feat, "features after the rasteriser's backward")


# ---- 7. both binning paths, both forward modes --------------------------------------------------------------------------
def test_binning_paths_and_forward_modes(native_lib):
    from monogs_amd import rasterizer as R, render_features
    sc = _scene("long")
    P, K = sc.means3D.shape[0], 16
    feat = _features(P, K).to(DEV)
    R.set_sync_free(False)
    assert native_lib.mgs_binning_path(P, W, H) == 0
    ref = render_features(_forward(sc)[0], feat)          # exact mode, global depth sort (records the capacity hint)
    with options(radix_scanned=1):
        assert native_lib.mgs_binning_path(P, W, H) == 1
        per_tile = render_features(_forward(sc)[0], feat)
    assert (per_tile - ref).abs().max() <= 1e-6
    try:
        R.set_sync_free(True, headroom=1.2)
        color = _forward(sc)[0]
        assert color.grad_fn.overflow is not None         # the capacity path ran
        cap = render_features(color, feat)
        assert not R.check_overflow()
    finally:
        R.set_sync_free(False)
        R.forget_capacity(P, W, H)
    assert (cap - ref).abs().max() <= 1e-6


# ---- 8. the stand-alone form --------------------------------------------------------------------------------------------
def test_feature_rasterizer(native_lib):
    from monogs_amd import FeatureRasterizer, render_features
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    sc = _scene("multi")
    K = 5
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    feat = _features(sc.means3D.shape[0], K).to(DEV).requires_grad_(True)
    res = FeatureRasterizer(st)(sc.means3D.to(DEV), sc.opacities.to(DEV), feat, scales=_scales(sc).to(DEV),
                                rotations=sc.rotations.to(DEV), want_labels=True)
    assert set(res) == {"features", "depth", "opacity", "radii", "n_touched", "labels"}
    color, radii, depth, opacity, _ = _forward(sc)
    ref, amb, _ = _oracle_forward("multi", K)
    _check_pixels(res["features"].detach().cpu(), ref, amb, "FeatureRasterizer")
    assert (res["features"] - render_features(color, feat)).abs().max() <= 1e-6
    assert (res["depth"] - depth).abs().max() <= 1e-6 and (res["opacity"] - opacity).abs().max() <= 1e-6
    assert torch.equal(res["radii"], radii)
    (res["features"] * _grad_out(K).to(DEV)).sum().backward()
    _check_grad(feat.grad, _oracle_backward("multi", K), "FeatureRasterizer backward")
    # no Gaussians: the background and no label
    bg = torch.tensor([0.2, 0.4, 0.6, 0.8, 1.0], device=DEV)
    e = lambda *s: torch.empty(*s, device=DEV)  # noqa: E731
    res0 = FeatureRasterizer(st)(e(0, 3), e(0, 1), e(0, K), scales=e(0, 3), rotations=e(0, 4), bg=bg, want_labels=True)
    assert torch.equal(res0["features"], bg[:, None, None].expand(K, H, W))
    assert (res0["labels"] == -1).all()
