"""``fused_ssim`` -- host side of the fused-ssim drop-in (HIP, forward value + analytic gradient).

Call sites: /root/reference/gaussian_splatting/utils/loss_utils.py:19 (``from fused_ssim import fused_ssim``) and :43-45
(``ssim(img1, img2) = fused_ssim(img1, img2, padding="valid")``), used by ``Mapper.refinement()``
(/root/reference/utils/slam_mapper.py:529-539, un-batched ``[3,H,W]`` images) and ``eval_rendering()``
(/root/reference/utils/eval_utils.py:183, ``[1,3,H,W]``).  The function is SSIM of Wang et al. 2004 with the 11-tap Gaussian
window of sigma 1.5 and zero padding (csrc/ssim.hip); upstream's extension is not available here, so parity with its binary
is unpinned.  The gradient goes to ``img1`` only.
"""
from __future__ import annotations

import torch

from . import _lib
from ._launch import _f32, _stream, _device_guard

C1, C2 = _lib.H.MGS_SSIM_C1, _lib.H.MGS_SSIM_C2          # 0.01 ** 2 and 0.03 ** 2: the same float32 bits
WINDOW = 11


def _check_pair(img1, img2, padding):
    """Argument errors, before anything touches a device.  Returns (planes, H, W, valid)."""
    if padding not in ("same", "valid"):
        raise ValueError(f"padding must be 'same' or 'valid' (got {padding!r})")
    if img1.shape != img2.shape:
        raise ValueError(f"img1 and img2 must have the same shape (got {tuple(img1.shape)} and {tuple(img2.shape)})")
    if img1.dim() not in (3, 4):
        raise ValueError(f"expected [B,C,H,W] or [C,H,W] images (got {tuple(img1.shape)})")
    H, W = int(img1.shape[-2]), int(img1.shape[-1])
    planes = int(img1.numel() // max(H * W, 1))
    if planes < 1 or H < 1 or W < 1:
        raise ValueError(f"empty image {tuple(img1.shape)}")
    valid = padding == "valid"
    if valid and (H < WINDOW or W < WINDOW):
        raise ValueError(f"padding='valid' needs at least {WINDOW} x {WINDOW} pixels (got {H} x {W}): nothing to average")
    if not (img1.is_cuda and img2.is_cuda):
        raise RuntimeError("fused_ssim expects CUDA/HIP tensors; there is no CPU path")
    return planes, H, W, valid


def _forward(img1, img2, planes, H, W, valid, train):
    """Launch the forward on the current stream: (value, scratch).  ``scratch`` carries the derivative planes when ``train``."""
    lib = _lib.load()
    dev = img1.device
    with _device_guard(dev):
        scratch = torch.empty(lib.mgs_ssim_scratch_bytes(planes, W, H, int(train)) // 4, dtype=torch.float32, device=dev)
        value = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.mgs_ssim_forward(planes, W, H, int(valid), int(train), C1, C2, img1.data_ptr(), img2.data_ptr(),
                                        scratch.data_ptr(), value.data_ptr(), _stream()), "mgs_ssim_forward")
    return value, scratch


class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, planes, H, W, valid):
        x, y = _f32(img1.detach(), "img1"), _f32(img2.detach(), "img2")
        value, scratch = _forward(x, y, planes, H, W, valid, True)
        ctx.cfg = (planes, H, W, valid)
        ctx.save_for_backward(x, y, scratch)
        return value

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        x, y, scratch = ctx.saved_tensors
        planes, H, W, valid = ctx.cfg
        with _device_guard(x.device):
            go = _f32(grad_out.reshape(1), "grad_output")
            d_img1 = torch.empty_like(x)
            _lib.check(lib.mgs_ssim_backward(planes, W, H, int(valid), C1, C2, x.data_ptr(), y.data_ptr(), scratch.data_ptr(),
                                             go.data_ptr(), d_img1.data_ptr(), _stream()), "mgs_ssim_backward")
        return d_img1, None, None, None, None, None


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same", train: bool = True) -> torch.Tensor:
    """Mean SSIM of ``img1`` against ``img2`` (``[B,C,H,W]``, or ``[C,H,W]`` as one image) as a 0-d float32 tensor on their
    device.  ``padding="same"`` averages the whole map, ``"valid"`` the map without its outer 5 pixels.  ``train=False``
    computes the same value without keeping anything for a backward."""
    planes, H, W, valid = _check_pair(img1, img2, padding)
    if train and torch.is_grad_enabled() and img1.requires_grad:
        return _FusedSSIM.apply(img1, img2, planes, H, W, valid)
    value, _ = _forward(_f32(img1.detach(), "img1"), _f32(img2.detach(), "img2"), planes, H, W, valid, False)
    return value
