"""Fused ``get_loss_mapping`` / ``get_loss_tracking`` (HIP, forward value + analytic gradients).

Same signatures and values as /root/reference/utils/slam_utils.py:58-146 (mirrored in plain PyTorch in
``oracle/slam_losses.py`` -- test infrastructure -- and checked there against the reference's own outputs); one reduction kernel
per forward and one elementwise kernel per backward instead of ~60 small kernels and two host syncs.
One difference, invisible to the rasteriser: the opacity image receives no gradient from the tracking loss (the
rasteriser ignores dL/dopacity anyway).  ``invert_depth`` (slam_utils.py:83-88, :138-141) is the mode bit
``MGS_LOSS_INVERT_DEPTH`` of the kernels.

Monocular frames (``get_loss_tracking_rgb`` / ``get_loss_mapping_rgb``, ``loss_grads(rgb_only=True)``): the mode bit
``MGS_LOSS_RGB_ONLY`` drops the depth term and its two images from the same kernels -- a [RECALL] of the two functions of that
name in public upstream MonoGS (the reference fork removed them), parity unpinned; DESIGN.md, "Monocular operation".
"""
from __future__ import annotations

import torch

from . import _lib
from ._launch import _f32, _stream, _device_guard


_TRACKING, _INVERT, _RGB_ONLY = _lib.H.MGS_LOSS_TRACKING, _lib.H.MGS_LOSS_INVERT_DEPTH, _lib.H.MGS_LOSS_RGB_ONLY
_DAB, _LOSS = _lib.H.MGS_LOSS_SCRATCH_DAB, _lib.H.MGS_LOSS_SCRATCH_LOSS        # float indices into the loss scratch


def _u8(t):
    if t is None:
        return None
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    return (t != 0).to(torch.uint8).contiguous()


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, depth, opacity, exp_a, exp_b, gt_rgb, gt_depth, mask, grad_mask, mode, init, lam):
        lib = _lib.load()
        render = _f32(render.detach(), "render_image")
        rgb_only = bool(int(mode) & _RGB_ONLY)        # neither depth image reaches the kernels
        depth = None if rgb_only else _f32(depth.detach(), "render_depth")
        H, W = render.shape[-2:]
        dev = render.device
        opac = _f32(opacity.detach(), "render_opacity") if opacity is not None else None
        gt_rgb, gt_depth = _f32(gt_rgb, "viewpoint.rgb"), None if rgb_only else _f32(gt_depth, "viewpoint.depth")
        a = _f32(exp_a.detach(), "exposure_a") if exp_a is not None else None
        b = _f32(exp_b.detach(), "exposure_b") if exp_b is not None else None
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with _device_guard(dev):
            scratch = torch.empty(lib.mgs_loss_scratch_bytes() // 4, dtype=torch.float32, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(lib.mgs_loss_forward(W, H, int(mode), int(init), float(lam), p(render), p(depth), p(opac),
                                            p(gt_rgb), p(gt_depth), p(mask), p(grad_mask), p(a), p(b),
                                            p(scratch), p(loss), _stream()), "mgs_loss_forward")
        ctx.cfg = (W, H, int(mode), int(init), float(lam))
        ctx.has_mask, ctx.has_gm, ctx.has_op, ctx.has_ab = mask is not None, grad_mask is not None, opac is not None, a is not None
        dummy = torch.empty(0, device=dev)
        ctx.save_for_backward(render, depth if depth is not None else dummy, opac if opac is not None else dummy, gt_rgb,
                              gt_depth if gt_depth is not None else dummy,
                              mask if mask is not None else dummy, grad_mask if grad_mask is not None else dummy,
                              a if a is not None else dummy, b if b is not None else dummy, scratch)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        render, depth, opac, gt_rgb, gt_depth, mask, gm, a, b, scratch = ctx.saved_tensors
        W, H, mode, init, lam = ctx.cfg
        dev = render.device
        p = lambda t, ok=True: t.data_ptr() if ok else None  # noqa: E731
        with _device_guard(dev):
            go = _f32(grad_out.reshape(1), "grad_output")
            d_render = torch.empty_like(render)
            rgb_only = bool(mode & _RGB_ONLY)
            # RGB-only: a render depth that asks for a gradient gets zeros (the kernel's memset node), otherwise nothing is written
            d_depth = (torch.empty(1, H, W, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None) if rgb_only \
                else torch.empty_like(depth)
            want_ab = ctx.has_ab and not init and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
            d_ab = None
            if want_ab:
                if getattr(ctx, "dab_used", False):        # a second backward of the same forward: separate, cleared buffer
                    d_ab = torch.empty(2, dtype=torch.float32, device=dev)
                else:                                      # the slot the forward left zeroed (MGS_LOSS_SCRATCH_DAB)
                    d_ab = scratch[_DAB:_DAB + 2]
                    ctx.dab_used = True
            _lib.check(lib.mgs_loss_backward(W, H, mode, init, lam, p(render), p(depth, not rgb_only), p(opac, ctx.has_op),
                                             p(gt_rgb), p(gt_depth, not rgb_only), p(mask, ctx.has_mask), p(gm, ctx.has_gm),
                                             p(a, ctx.has_ab), p(b, ctx.has_ab), p(scratch), p(go), p(d_render),
                                             p(d_depth, d_depth is not None), d_ab.data_ptr() if d_ab is not None else None, _stream()),
                       "mgs_loss_backward")
        d_a = d_ab[0:1] if d_ab is not None else None      # views: autograd takes them as .grad without a copy kernel
        d_b = d_ab[1:2] if d_ab is not None else None
        return (d_render, d_depth, None, d_a, d_b, None, None, None, None, None, None, None)


def get_loss_mapping(render_image, render_depth, viewpoint, init=False, invert_depth=False, lambda_depth=0.9):
    return _FusedLoss.apply(render_image, render_depth, None, viewpoint.exposure_a, viewpoint.exposure_b,
                            viewpoint.rgb, viewpoint.depth, _u8(viewpoint.mask), None,
                            _INVERT if invert_depth else 0, bool(init), float(lambda_depth))


def get_loss_tracking(render_image, render_depth, render_opacity, viewpoint, invert_depth=False, lambda_depth=0.9):
    return _FusedLoss.apply(render_image, render_depth, render_opacity, viewpoint.exposure_a, viewpoint.exposure_b,
                            viewpoint.rgb, viewpoint.depth, _u8(viewpoint.mask), _u8(viewpoint.grad_mask),
                            _TRACKING | (_INVERT if invert_depth else 0), False, 0.9)


def get_loss_tracking_rgb(render_image, render_depth, render_opacity, viewpoint):
    """The tracking loss of a monocular frame: ``get_loss_tracking`` without its depth term.  ``render_depth`` is not read (it
    gets a zero gradient if it asks for one); ``viewpoint.depth`` is not read either."""
    return _FusedLoss.apply(render_image, render_depth, render_opacity, viewpoint.exposure_a, viewpoint.exposure_b,
                            viewpoint.rgb, None, _u8(viewpoint.mask), _u8(viewpoint.grad_mask), _TRACKING | _RGB_ONLY, False, 1.0)


def get_loss_mapping_rgb(render_image, render_depth, viewpoint, init=False):
    """The mapping loss of a monocular frame: the masked L1 of the colour image alone, coefficient 1."""
    return _FusedLoss.apply(render_image, render_depth, None, viewpoint.exposure_a, viewpoint.exposure_b,
                            viewpoint.rgb, None, _u8(viewpoint.mask), None, _RGB_ONLY, bool(init), 1.0)


class LossGrads:
    """Result of ``loss_grads``: upstream gradients for the rasteriser + views of the scalar results on the device.
    ``d_depth`` is None for an RGB-only loss: ``backward`` then drives the colour image alone."""
    __slots__ = ("d_render", "d_depth", "scratch", "has_exposure")

    def __init__(self, d_render, d_depth, scratch, has_exposure):
        self.d_render, self.d_depth, self.scratch, self.has_exposure = d_render, d_depth, scratch, has_exposure

    @property
    def loss(self) -> torch.Tensor:                    # device scalar, valid once the two kernels have run
        return self.scratch[_LOSS]

    @property
    def d_exposure_a(self):
        return self.scratch[_DAB:_DAB + 1] if self.has_exposure else None

    @property
    def d_exposure_b(self):
        return self.scratch[_DAB + 1:_DAB + 2] if self.has_exposure else None

    def backward(self, render_image, render_depth, viewpoint=None, accumulate=False):
        """Drive the rasteriser's backward with these gradients and hand the exposure gradients to the viewpoint."""
        if self.d_depth is None:
            torch.autograd.backward([render_image], [self.d_render])
        else:
            torch.autograd.backward([render_image, render_depth], [self.d_render, self.d_depth])
        if viewpoint is not None and self.has_exposure:
            for p, g in ((viewpoint.exposure_a, self.d_exposure_a), (viewpoint.exposure_b, self.d_exposure_b)):
                p.grad = g if (p.grad is None or not accumulate) else p.grad + g


@torch.no_grad()
def loss_grads(render_image, render_depth, render_opacity, viewpoint, tracking: bool, init: bool = False,
               lambda_depth: float = 0.9, invert_depth: bool = False, rgb_only: bool = False) -> LossGrads:
    """``get_loss_tracking`` / ``get_loss_mapping`` (/root/reference/utils/slam_utils.py:58-146) as VALUE + GRADIENTS in two
    launches, for loops that call the rasteriser's backward themselves: no autograd node for the scalar, hence no finalize
    kernel, no ones-fill and no loss-summing adds (``loss.backward()`` on the fused autograd loss costs four launches per
    render).  Same numbers as ``_FusedLoss`` forward + backward with grad_output = 1.
    ``rgb_only``: the monocular losses (``get_loss_tracking_rgb`` / ``get_loss_mapping_rgb``): ``render_depth`` and
    ``viewpoint.depth`` are not read and ``d_depth`` is None."""
    lib = _lib.load()
    render = _f32(render_image.detach(), "render_image")
    depth = None if rgb_only else _f32(render_depth.detach(), "render_depth")
    H, W = render.shape[-2:]
    dev = render.device
    opac = _f32(render_opacity.detach(), "render_opacity") if tracking else None
    gt_rgb, gt_depth = _f32(viewpoint.rgb, "viewpoint.rgb"), None if rgb_only else _f32(viewpoint.depth, "viewpoint.depth")
    a = None if init else _f32(viewpoint.exposure_a.detach(), "exposure_a")
    b = None if init else _f32(viewpoint.exposure_b.detach(), "exposure_b")
    mask = _u8(viewpoint.mask)
    gm = _u8(viewpoint.grad_mask) if tracking else None
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with _device_guard(dev):
        scratch = torch.empty(lib.mgs_loss_scratch_bytes() // 4, dtype=torch.float32, device=dev)
        d_render, d_depth = torch.empty_like(render), None if rgb_only else torch.empty_like(depth)
        mode = (_TRACKING if tracking else 0) | (_INVERT if invert_depth else 0) | (_RGB_ONLY if rgb_only else 0)
        _lib.check(lib.mgs_loss_grads(W, H, mode, int(init), 0.9 if tracking else float(lambda_depth), p(render),
                                      p(depth), p(opac), p(gt_rgb), p(gt_depth), p(mask), p(gm), p(a), p(b), p(scratch),
                                      p(d_render), p(d_depth), _stream()), "mgs_loss_grads")
    return LossGrads(d_render, d_depth, scratch, not init)


# ---- colour refinement: (1 - lambda) L1 + lambda (1 - SSIM) ------------------------------------------------------------------
_R_LOSS, _R_L1, _R_SSIM = _lib.H.MGS_SSIM_SCRATCH_LOSS, _lib.H.MGS_SSIM_SCRATCH_L1, _lib.H.MGS_SSIM_SCRATCH_SSIM


def _refine_inputs(image, gt_image):
    from .ssim import _check_pair
    if image.dim() == 4 and image.shape[0] == 1:
        image = image[0]
    if gt_image.dim() == 4 and gt_image.shape[0] == 1:
        gt_image = gt_image[0]
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"the refinement loss takes one [3,H,W] image (got {tuple(image.shape)})")
    _, H, W, _ = _check_pair(image, gt_image, "valid")
    return _f32(image.detach(), "image"), _f32(gt_image.detach(), "gt_image"), H, W


class _RefineLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt_image, lam):
        lib = _lib.load()
        render, gt, H, W = _refine_inputs(image, gt_image)
        dev = render.device
        with _device_guard(dev):
            scratch = torch.empty(lib.mgs_ssim_scratch_bytes(3, W, H, 1) // 4, dtype=torch.float32, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(lib.mgs_refine_loss_forward(W, H, lam, render.data_ptr(), gt.data_ptr(), scratch.data_ptr(),
                                                   loss.data_ptr(), _stream()), "mgs_refine_loss_forward")
        ctx.cfg = (W, H, lam, tuple(image.shape))
        ctx.save_for_backward(render, gt, scratch)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        render, gt, scratch = ctx.saved_tensors
        W, H, lam, shape = ctx.cfg
        with _device_guard(render.device):
            go = _f32(grad_out.reshape(1), "grad_output")
            d_render = torch.empty_like(render)
            _lib.check(lib.mgs_refine_loss_backward(W, H, lam, render.data_ptr(), gt.data_ptr(), scratch.data_ptr(),
                                                    go.data_ptr(), d_render.data_ptr(), _stream()), "mgs_refine_loss_backward")
        return d_render.view(shape), None, None


def get_loss_refinement(image, gt_image, lambda_ssim=0.2):
    """The loss of ``Mapper.refinement()`` (/root/reference/utils/slam_mapper.py:529-539) as one autograd scalar:
    ``(1 - lambda) |image - gt|.mean() + lambda (1 - ssim(image, gt))`` with the reference's ``ssim`` (``padding="valid"``).
    One forward kernel + finalize, one backward kernel (csrc/ssim.hip); gradient to ``image`` only."""
    return _RefineLoss.apply(image, gt_image, float(lambda_ssim))


class RefineGrads:
    """Result of ``refinement_loss_grads``: dL/dimage + views of the scalar results on the device."""
    __slots__ = ("d_render", "scratch")

    def __init__(self, d_render, scratch):
        self.d_render, self.scratch = d_render, scratch

    @property
    def loss(self) -> torch.Tensor:
        return self.scratch[_R_LOSS]

    @property
    def l1(self) -> torch.Tensor:
        return self.scratch[_R_L1]

    @property
    def ssim(self) -> torch.Tensor:
        return self.scratch[_R_SSIM]

    def backward(self, image):
        torch.autograd.backward([image], [self.d_render.view(image.shape)])


@torch.no_grad()
def refinement_loss_grads(image, gt_image, lambda_ssim=0.2) -> RefineGrads:
    """``get_loss_refinement`` as VALUE + GRADIENT (for grad_output = 1) in three launches and no host synchronisation, for
    loops that call ``torch.autograd.backward([image], [d_render])`` themselves, as ``loss_grads`` does for the SLAM losses.
    Same numbers as the autograd path, bit for bit."""
    lib = _lib.load()
    render, gt, H, W = _refine_inputs(image, gt_image)
    dev = render.device
    with _device_guard(dev):
        scratch = torch.empty(lib.mgs_ssim_scratch_bytes(3, W, H, 1) // 4, dtype=torch.float32, device=dev)
        d_render = torch.empty_like(render)
        _lib.check(lib.mgs_refine_loss_grads(W, H, float(lambda_ssim), render.data_ptr(), gt.data_ptr(), scratch.data_ptr(),
                                             d_render.data_ptr(), _stream()), "mgs_refine_loss_grads")
    return RefineGrads(d_render, scratch)
