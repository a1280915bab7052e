"""``mgs_image_metrics`` (csrc/metrics.hip) through ``monogs_amd.evaluation.image_metrics`` on the GPU (pytest -m gpu).

Bars: the clamped image, the channels-last bytes and the count are exact; the MSE is within 1e-5 relative of a float64
evaluation of the same float32 inputs (hence the PSNR within 10 log10(1 + 1e-5) = 4.4e-5 dB) -- the kernel carries its sums in
double, its own bound is 2.4e-7 + one float rounding; the SSIM slot equals ``fused_ssim`` bitwise; two calls agree bitwise."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(11, 11), (11, 13), (12, 17), (37, 53), (64, 64), (121, 67)]      # (H, W); 12 x 17 and 64 x 64 take the 16-byte path
KINDS = ("masked", "gt_all_zero", "render_equals_gt")


def _inputs(kind, H, W, offset):
    """(render, gt) as [3,H,W] float32 views that start ``offset`` floats into a larger buffer (1: no 16-byte alignment)."""
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + KINDS.index(kind))
    n = 3 * H * W
    gt = torch.rand(n, generator=gen)
    gt[torch.rand(n, generator=gen) < 0.2] = 0.0                            # about 20 % exactly zero: outside the PSNR mask
    render = torch.rand(n, generator=gen) * 1.6 - 0.3                       # [-0.3, 1.3]: the clamp acts on both sides
    if kind == "gt_all_zero":
        gt.zero_()
    elif kind == "render_equals_gt":
        render = gt.clone()

    def view(t):
        buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
        v = buf[offset:offset + n].view(3, H, W)
        v.copy_(t.view(3, H, W))
        assert v.data_ptr() % 16 == (4 * offset) % 16
        return v
    return view(render), view(gt)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_metrics(native_lib, size, kind, offset):
    from fused_ssim import fused_ssim
    from monogs_amd.evaluation import image_metrics
    H, W = size
    render, gt = _inputs(kind, H, W, offset)
    n = 3 * H * W
    out_buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=DEV)
    clamped_out = out_buf[offset:offset + n].view(3, H, W)
    row = torch.full((4,), -7.0, dtype=torch.float32, device=DEV)
    row, clamped, u8 = image_metrics(render, gt, row=row, want_u8=True, clamped_out=clamped_out)
    want_c = torch.clamp(render, 0.0, 1.0)
    assert clamped.data_ptr() == clamped_out.data_ptr() and torch.equal(clamped, want_c)
    assert bool(torch.isnan(out_buf[:offset]).all()) and bool(torch.isnan(out_buf[offset + n:]).all())      # nothing written outside
    assert u8.shape == (H, W, 3) and torch.equal(u8, (want_c * 255).to(torch.uint8).permute(1, 2, 0).contiguous())
    psnr, ssim, mse, count = (float(v) for v in row.cpu())
    mask = gt > 0
    assert count == float(mask.sum()), (count, int(mask.sum()))
    if kind == "gt_all_zero":
        assert count == 0 and math.isnan(mse) and math.isnan(psnr)
    else:
        assert 0.7 * n < count < 0.9 * n
        mse64 = float(((want_c.double() - gt.double())[mask] ** 2).mean())
        if kind == "render_equals_gt":
            assert mse64 == 0.0 and mse == 0.0 and psnr == float("inf")
        else:
            rel = abs(mse - mse64) / mse64
            psnr64 = 20.0 * math.log10(1.0 / math.sqrt(mse64))
            print(f"{H}x{W} offset {offset}: mse rel err {rel:.3g} (bar 1e-5), psnr err {abs(psnr - psnr64):.3g} dB (bar 4.4e-5)")
            assert rel <= 1e-5, (mse, mse64)
            assert abs(psnr - psnr64) <= 4.4e-5, (psnr, psnr64)
    # slot 1 is the SSIM call on the clamped image, bit for bit
    want_s = fused_ssim(want_c[None].contiguous(), gt[None].contiguous(), padding="valid", train=False)
    assert torch.equal(row[1], want_s), (float(row[1]), float(want_s))
    # bitwise reproducible, and without the optional outputs the same row
    row2, _, none = image_metrics(render, gt)
    assert none is None and torch.equal(row2.view(torch.int32), row.view(torch.int32))
