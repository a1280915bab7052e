"""The fused label loss and the confusion count (csrc/labels.hip, monogs_amd/object_layer.py) against the float64 mirror
(tests/object_layer_mirror.py) on the same float32 inputs.  Run on the MI355X box: pytest -m gpu.

Shapes: one pixel, sizes below one workgroup, an odd W (the scalar route), W % 4 == 0 (the 16-byte route), several workgroups
with a ragged tail.  K: 1..3 and 16..18 sit in the two register chunks (<= 8, <= 24), 64 / 255 / 256 take the two-pass form.
Tolerances: the loss is held to the project's bar for its fused losses (tests/test_gpu_losses.py), |L - L64| <= 2e-6 max(1, |L64|);
the gradient to |g - g64| <= 1e-4 |g64| + 4 * 2^-24 / N -- the relative part is the project's gradient bar, the absolute part a few
float32 units of a probability near 1, which softmax - 1 at the label cannot do better than, divided by N as the gradient is."""
import functools

import numpy as np
import pytest
import torch

from object_layer_mirror import confusion_mirror, counted_mask, label_loss_mirror

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (3, 5), (23, 37), (48, 64), (120, 160)]
KS = [1, 2, 3, 16, 17, 18, 64, 255, 256]
CASES = [(H, W, 18) for H, W in SHAPES] + [(H, W, K) for H, W in ((23, 37), (48, 64)) for K in KS if K != 18]


@functools.lru_cache(maxsize=None)
def _inputs(H, W, K, kind="plain"):
    """(feat float32 [K,H,W], labels int64 [H,W], valid uint8 [H,W] or None) on the CPU; labels include ids >= K where 8 bits allow."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + K)
    feat = 3.0 * torch.randn(K, H, W, generator=g)
    labels = torch.randint(0, min(K + 2, 256), (H, W), generator=g)
    if K < 256 and H * W > 1:
        labels[-1, -1] = K                      # whatever the draw: one id the loss has no channel for
    valid = None
    if kind == "half":
        valid = (torch.rand(H, W, generator=g) < 0.5).to(torch.uint8)
    elif kind == "none":
        valid = torch.zeros(H, W, dtype=torch.uint8)
    elif kind == "one":
        valid = torch.zeros(H, W, dtype=torch.uint8)
        valid[H // 2, W // 3] = 1
        labels[H // 2, W // 3] = K - 1
    elif kind == "large":
        feat = 1e4 * (torch.randint(0, 3, (K, H, W), generator=g) - 1).float()
    return feat, labels, valid


@functools.lru_cache(maxsize=None)
def _mirror(H, W, K, kind="plain"):
    return label_loss_mirror(*_inputs(H, W, K, kind))


def _run(feat_dev, labels, valid):
    from monogs_amd.object_layer import LabelTarget, label_loss_grads
    target = LabelTarget(labels.to(DEV), None if valid is None else valid.to(DEV))
    g = label_loss_grads(feat_dev, target)
    return g, target


def _check(g, mirror, labels, valid, K, what):
    L64, d64, N = mirror
    L, d = float(g.loss), g.d_feat.cpu().double()
    assert int(g.count) == N, what
    err_L = abs(L - float(L64))
    err_g = (d - d64).abs()
    bound = 1e-4 * d64.abs() + 4 * 2.0 ** -24 / max(N, 1)
    print(f"{what}: N {N}, L {L:.7f} (float64 {float(L64):.7f}, diff {err_L:.2e}), worst gradient error / bound "
          f"{float((err_g / bound).max()):.3f}")
    assert torch.isfinite(g.d_feat).all() and np.isfinite(L), what
    assert err_L <= 2e-6 * max(1.0, abs(float(L64))), what
    assert (err_g <= bound).all(), what
    off = ~counted_mask(labels, valid, K)
    assert (g.d_feat.cpu()[:, off] == 0).all(), what           # exactly 0 on every pixel that is not counted


@pytest.mark.parametrize("H,W,K", CASES)
def test_loss_and_gradient_match_the_mirror(native_lib, H, W, K):
    from monogs_amd.object_layer import label_loss_grads
    feat, labels, valid = _inputs(H, W, K)
    f = feat.to(DEV)
    g, target = _run(f, labels, valid)
    _check(g, _mirror(H, W, K), labels, valid, K, f"{H}x{W} K={K}")
    if K < 256 and H * W > 1:
        assert (labels >= K).any() and not counted_mask(labels, valid, K).all()       # ids >= K are present and ignored
    again = label_loss_grads(f, target)                         # bit-identical from call to call
    assert torch.equal(again.loss, g.loss) and torch.equal(again.d_feat, g.d_feat)


def test_alignment_chooses_the_route_not_the_shape(native_lib):
    """W % 4 == 0 but the image starts one float into its buffer: the scalar route, same numbers."""
    H, W, K = 48, 64, 18
    feat, labels, valid = _inputs(H, W, K)
    buf = torch.empty(K * H * W + 1, device=DEV)
    view = buf[1:].view(K, H, W)
    view.copy_(feat)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    g, _ = _run(view, labels, valid)
    _check(g, _mirror(H, W, K), labels, valid, K, "view offset by one float")
    aligned, _ = _run(feat.to(DEV), labels, valid)
    assert (g.d_feat - aligned.d_feat).abs().max() <= 2.0 ** -24 / g.count.item() * 4


@pytest.mark.parametrize("kind", ["half", "none", "one", "large"])
@pytest.mark.parametrize("H,W", [(23, 37), (48, 64)])
def test_valid_images_and_large_logits(native_lib, H, W, kind):
    K = 18
    feat, labels, valid = _inputs(H, W, K, kind)
    g, _ = _run(feat.to(DEV), labels, valid)
    _check(g, _mirror(H, W, K, kind), labels, valid, K, f"{H}x{W} {kind}")
    if kind == "none":
        assert int(g.count) == 0 and float(g.loss) == 0.0 and (g.d_feat == 0).all()
    if kind == "one":
        assert int(g.count) == 1 and int((g.d_feat != 0).any(0).sum()) == 1
    if kind == "half":
        assert 0.3 < float(valid.float().mean()) < 0.7


@pytest.mark.parametrize("H,W", [(23, 37), (48, 64)])
def test_one_channel_is_exactly_zero(native_lib, H, W):
    feat, labels, valid = _inputs(H, W, 1)
    g, _ = _run(feat.to(DEV), labels, valid)
    assert int(g.count) == int((labels < 1).sum()) > 0
    assert float(g.loss) == 0.0 and (g.d_feat == 0).all()


def test_autograd_form_scales_the_same_image(native_lib):
    from monogs_amd.object_layer import get_loss_labels
    H, W, K = 23, 37, 18
    feat, labels, valid = _inputs(H, W, K, "half")
    f = feat.to(DEV).requires_grad_(True)
    g, target = _run(f.detach(), labels, valid)
    loss = get_loss_labels(f, target)
    assert torch.equal(loss.detach(), g.loss)
    (loss * 2.5).backward()
    assert torch.equal(f.grad, g.d_feat * 2.5)


@pytest.mark.parametrize("H,W", [(23, 37), (120, 160)])
@pytest.mark.parametrize("K", [1, 2, 18, 64, 256])
def test_confusion_counts_are_exact(native_lib, H, W, K):
    from monogs_amd.object_layer import LabelTarget, label_confusion
    g = torch.Generator().manual_seed(7 * H + K)
    gt = torch.randint(0, min(K + 2, 256), (H, W), generator=g)
    pred = torch.randint(-1, K, (H, W), generator=g).to(torch.int32)
    # a confident predictor: most pixels on the diagonal, so that a few cells are hot
    agree = torch.rand(H, W, generator=g) < 0.6
    pred = torch.where(agree & (gt < K), gt.to(torch.int32), pred)
    valid = (torch.rand(H, W, generator=g) < 0.8).to(torch.uint8)
    counts64, side64 = confusion_mirror(pred, gt, valid, K)
    assert side64[0] > 0 and side64[1] > 0                      # -1 predictions and ignored pixels are present
    target = LabelTarget(gt.to(DEV), valid.to(DEV))
    out = label_confusion(pred.to(DEV), target, K)
    for rep in (1, 2):                                          # a second call into the same `out` doubles every entry
        counts, side = (t.cpu().numpy().view(np.uint32).astype(np.int64) for t in out)
        assert np.array_equal(counts, rep * counts64), (K, rep)
        assert np.array_equal(side, rep * side64), (K, rep)
        assert counts.sum() + side.sum() == rep * H * W
        if rep == 1:
            assert label_confusion(pred.to(DEV), target, K, out=out) is out
