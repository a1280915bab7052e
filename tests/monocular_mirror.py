"""TEST INFRASTRUCTURE: a float64 restatement of the monocular specification ("Monocular operation") in plain PyTorch.

The two RGB-only losses and the depth hypothesis of a keyframe without measured depth are a [RECALL] of public upstream MonoGS
(``get_loss_tracking_rgb``, ``get_loss_mapping_rgb``, ``add_new_keyframe``); the reference fork removed them, so nothing of it can be
run to pin them.  What it does keep -- ``get_median_depth(..., return_std=True)`` and the RGB-D losses -- pins the pieces this
mirror is made of (tests/test_monocular_host.py).  The inputs come from a fixed recipe so that every test sees the same data."""
import types

import torch

SIZES = [(48, 64), (47, 61)]          # H*W % 4 == 0: the 4-pixel path; odd H*W: the scalar path
SEEDS = [0, 1, 2, 3]
PARAMS = dict(init_mean=2.0, init_sigma=0.3, opacity_min=0.95, sigma_in=0.2, sigma_out=0.5)


def recipe(H, W, seed):
    """(depth, opacity, valid_rgb, noise): float32 / bool CPU tensors [H,W]."""
    g = torch.Generator().manual_seed(seed)
    depth = 1 + 3 * torch.rand(H, W, generator=g)
    depth[:, :W // 8] = 0
    opacity = 0.9 + 0.1 * torch.rand(H, W, generator=g)
    valid_rgb = torch.rand(H, W, generator=g) > 0.1
    noise = torch.randn(H, W, generator=g)
    return depth, opacity, valid_rgb, noise


def loss_inputs(H, W, seed, device="cpu"):
    """A monocular viewpoint (zero depth, a mask with empty rows, non-zero exposure) and a render: ``(vp, render, depth, opacity)``."""
    g = torch.Generator().manual_seed(100 + seed)
    mask = torch.rand(H, W, generator=g) > 0.1
    mask[3:6] = False
    mask[H - 1] = False
    vp = types.SimpleNamespace(
        rgb=torch.rand(3, H, W, generator=g).to(device), depth=torch.zeros(H, W, device=device), sensor="monocular",
        mask=mask.to(device), grad_mask=(torch.rand(H, W, generator=g) > 0.4).to(device),
        exposure_a=torch.tensor([0.07], device=device, requires_grad=True),
        exposure_b=torch.tensor([-0.03], device=device, requires_grad=True))
    render = torch.rand(3, H, W, generator=g).to(device).requires_grad_(True)
    rdepth = (torch.rand(1, H, W, generator=g) * 3).to(device).requires_grad_(True)
    op = torch.rand(1, H, W, generator=g)
    op[torch.rand(1, H, W, generator=g) < 0.6] = 0.995
    return vp, render, rdepth, op.to(device)


def _f64(t):
    return t.detach().double()


def _exposed(render, vp, init, a, b):
    return render if init else torch.exp(a) * render + b


def tracking_rgb(render, opacity, vp, exposure=None):
    """L = 0.5 mean(opacity) mean_{3HW}(m |rgb - gt|), m = mask grad_mask (opacity > 0.99), in float64.  ``exposure``: (a, b) leaves
    to differentiate with respect to (default: the viewpoint's values, detached)."""
    a, b = exposure if exposure is not None else (_f64(vp.exposure_a), _f64(vp.exposure_b))
    rgb = _exposed(render, vp, False, a, b)
    op = _f64(opacity)
    m = (vp.mask.bool() & vp.grad_mask.bool() & (opacity[0] > 0.99)).double()
    return 0.5 * op.mean() * (m[None] * (rgb - _f64(vp.rgb)).abs()).mean()


def mapping_rgb(render, vp, init=False, exposure=None):
    """L = mean_{mask, 3 channels} |rgb - gt| in float64 (coefficient 1)."""
    a, b = exposure if exposure is not None else (_f64(vp.exposure_a), _f64(vp.exposure_b))
    rgb = _exposed(render, vp, init, a, b)
    return (rgb - _f64(vp.rgb)).abs()[:, vp.mask.bool()].mean()


def loss_and_grads(kind, render, opacity, vp, init=False):
    """(loss, d_render, d_exposure_a, d_exposure_b) of the mirror in float64 (the exposure gradients None when ``init``)."""
    r = _f64(render).requires_grad_(True)
    a, b = _f64(vp.exposure_a).requires_grad_(True), _f64(vp.exposure_b).requires_grad_(True)
    loss = tracking_rgb(r, opacity, vp, (a, b)) if kind == "tracking" else mapping_rgb(r, vp, init, (a, b))
    gs = torch.autograd.grad(loss, [r] if init else [r, a, b])
    return (loss.detach(), gs[0]) + ((None, None) if init else (gs[1], gs[2]))


def valid_set(depth, opacity, valid_rgb, opacity_min=PARAMS["opacity_min"]):
    v = depth > 0
    if opacity is not None:
        v = v & (opacity > opacity_min)
    if valid_rgb is not None:
        v = v & valid_rgb.bool()
    return v


def pseudo_depth(depth, opacity, valid_rgb, noise, dtype=torch.float64, **params):
    """The depth hypothesis in ``dtype`` arithmetic: ``dict(depth, median, std, count, used_init_rule, outlier, valid)``.
    ``depth=None``: the init rule."""
    p = dict(PARAMS, **params)
    z = noise.to(dtype)
    ok = torch.ones_like(noise, dtype=torch.bool) if valid_rgb is None else valid_rgb.bool()
    zero = torch.zeros_like(z)
    count = 0
    if depth is not None:
        valid = valid_set(depth, opacity, valid_rgb, p["opacity_min"])
        count = int(valid.sum())
    if depth is None or count < 2:
        out = torch.where(ok, p["init_mean"] + p["init_sigma"] * z, zero)
        return dict(depth=out, median=p["init_mean"], std=p["init_sigma"], count=count, used_init_rule=True, outlier=None,
                    valid=None if depth is None else valid)
    d = depth.to(dtype)
    sel = d[valid]
    median, std = sel.median(), sel.std()                   # torch.median: the lower median; torch.std: unbiased
    outlier = (d > median + std) | (d < median - std) | ~valid
    out = torch.where(outlier, median, d) + z * torch.where(outlier, p["sigma_out"], p["sigma_in"]) * std
    return dict(depth=torch.where(ok, out, zero), median=median, std=std, count=count, used_init_rule=False, outlier=outlier,
                valid=valid)


def decision_margin(depth, median, std, valid):
    """min over the valid pixels of ||d - median| - std| / std: how far the nearest pixel is from changing sides."""
    d = depth.double()[valid]
    return float((((d - float(median)).abs() - float(std)).abs() / float(std)).min())
