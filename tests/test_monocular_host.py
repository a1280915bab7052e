"""The float64 mirror of the monocular specification (tests/monocular_mirror.py) against what the reference pins: its median /
standard deviation helper (``oracle.slam_losses.get_median_depth``, itself pinned by tests/golden/median_depth.npz) and the RGB-D
losses (``oracle.slam_losses``, pinned by tests/golden/losses.npz) at the settings where their depth terms vanish.  CPU only."""
import types

import pytest
import torch

import monocular_mirror as mm
from oracle import slam_losses as S

CASES = [(H, W, s) for H, W in mm.SIZES for s in mm.SEEDS]


@pytest.mark.parametrize("H,W,seed", CASES)
def test_mirror_statistics_equal_the_reference_helper(H, W, seed):
    depth, opacity, valid_rgb, noise = mm.recipe(H, W, seed)
    m = mm.pseudo_depth(depth, opacity, valid_rgb, noise)
    med, std, valid = S.get_median_depth(depth, (opacity > 0.95) & valid_rgb, return_std=True)
    assert torch.equal(m["valid"], valid) and m["count"] == int(valid.sum()) >= 2
    assert float(m["median"]) == float(med)                     # an element of the data: the same one in either precision
    # torch's float32 std against the float64 one: a few roundings of 2^-24 over a two-pass sum
    assert abs(float(m["std"]) - float(std)) <= 1e-6 * float(m["std"])


@pytest.mark.parametrize("H,W,seed", CASES)
def test_recipe_keeps_every_outlier_decision_away_from_its_threshold(H, W, seed):
    """What lets the GPU test compare the outlier SETS without an exemption: no pixel closer than 2e-5 (relative to std) to either
    threshold, and float32 arithmetic deciding every pixel as float64 does."""
    depth, opacity, valid_rgb, noise = mm.recipe(H, W, seed)
    m64 = mm.pseudo_depth(depth, opacity, valid_rgb, noise)
    m32 = mm.pseudo_depth(depth, opacity, valid_rgb, noise, dtype=torch.float32)
    assert mm.decision_margin(depth, m64["median"], m64["std"], m64["valid"]) >= 2e-5
    assert torch.equal(m64["outlier"], m32["outlier"])
    assert bool((m64["depth"][~valid_rgb] == 0).all()) and bool((m64["depth"][valid_rgb] != 0).all())
    assert 0 < int(m64["outlier"].sum()) < H * W                # both branches are exercised


def test_mirror_init_rule():
    depth, opacity, valid_rgb, noise = mm.recipe(48, 64, 0)
    want = torch.where(valid_rgb, 2.0 + 0.3 * noise.double(), torch.zeros(48, 64, dtype=torch.float64))
    for m in (mm.pseudo_depth(None, None, valid_rgb, noise), mm.pseudo_depth(depth, torch.zeros_like(opacity), valid_rgb, noise)):
        assert m["used_init_rule"] and torch.equal(m["depth"], want)
    one = torch.zeros_like(depth)
    one[20, 30] = 2.5
    m = mm.pseudo_depth(one, torch.ones_like(opacity), None, noise)
    assert m["used_init_rule"] and m["count"] == 1 and torch.equal(m["depth"], 2.0 + 0.3 * noise.double())


def _as64(vp, **over):
    d = dict(rgb=vp.rgb.double(), depth=vp.depth.double(), mask=vp.mask, grad_mask=vp.grad_mask,
             exposure_a=vp.exposure_a.detach().double(), exposure_b=vp.exposure_b.detach().double())
    d.update(over)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("H,W", mm.SIZES)
def test_mirror_tracking_loss_is_the_reference_loss_on_zero_depth(H, W):
    vp, render, rdepth, op = mm.loss_inputs(H, W, 0)
    ref = S.get_loss_tracking(render.detach().double(), rdepth.detach().double(), op.double(), _as64(vp))
    got = mm.tracking_rgb(render.detach().double(), op, vp)
    assert float(ref) > 0 and abs(float(got) - float(ref)) <= 1e-14 * float(ref)


@pytest.mark.parametrize("H,W", mm.SIZES)
@pytest.mark.parametrize("init", [False, True])
def test_mirror_mapping_loss_is_the_reference_rgb_term(H, W, init):
    """``lambda_depth = 1`` leaves the reference's colour term alone (its depth term, over an all-positive depth, times zero)."""
    vp, render, rdepth, _ = mm.loss_inputs(H, W, 1)
    ref = S.get_loss_mapping(render.detach().double(), rdepth.detach().double(), _as64(vp, depth=torch.ones(H, W, dtype=torch.float64)),
                             init=init, lambda_depth=1.0)
    got = mm.mapping_rgb(render.detach().double(), vp, init=init)
    assert float(ref) > 0 and abs(float(got) - float(ref)) <= 1e-14 * float(ref)
    # and the gap the RGB-only mode closes: on a frame without depth the reference's mapping loss is 0 / 0
    assert torch.isnan(S.get_loss_mapping(render.detach().double(), rdepth.detach().double(), _as64(vp), init=init))
