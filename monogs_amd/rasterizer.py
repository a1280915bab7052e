"""``GaussianRasterizationSettings`` / ``GaussianRasterizer`` -- host side of the drop-in.

Mirrors the Python surface of the un-vendored ``diff_gaussian_rasterization`` (w-pose variant)
exactly as MonoGS uses it: settings built at
/root/reference/gaussian_splatting/gaussian_renderer/__init__.py:70-84, rasteriser called by
keyword at :130-156, outputs consumed at :160-168.  The arithmetic lives in
libmonogs_raster.so (HIP, gfx950) behind the C ABI of include/monogs_raster.h; torch is used
for device memory, the current stream and autograd plumbing only.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib
from ._launch import _device_guard, _f32, _ptr, _raw_stream, _stream  # noqa: F401  (re-exported: tests and tools import them here)
from .raster_status import (GraphFlags, StatusLedger, STATUS_CAPACITY_OVERFLOW,  # noqa: F401  (re-exported)
                            STATUS_DEPTH_SORT_TIMEOUT, STATUS_TILE_SORT_TIMEOUT)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    projmatrix_raw: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


# ---- sync-free ("capacity") mode ----------------------------------------------------------------
# The exact path (the default: what an unmodified MonoGS gets) reads the instance count R back to the host once per
# forward, as upstream does, to size the binning scratch.  It keeps ONE thing between calls: the status word of the last
# exact forward, which the next forward's count read-back collects at its own synchronisation, so that a radix-sort
# look-back timeout -- the one failure of the exact path -- is raised one forward later instead of never.
#
# Capacity mode is opt-in (`set_sync_free(True)`, or implied by a hipGraph capture): the scratch is sized from the LAST count
# seen for the same (P, W, H) times a headroom factor, the kernels read the live count on the device, and nothing in forward +
# backward synchronises the host -- which is what lets a whole tracking / mapping iteration be captured in a hipGraph.  An
# overflow (R > capacity) drops instances and sets a device flag; `check_overflow()` (one sync, e.g. next to the convergence
# test of the pose step) reports it and raises the capacity so the caller can redo the iteration.
#
# What is remembered between calls -- the hints, the unread words -- lives in ONE `raster_status.StatusLedger` (`_ledger`);
# its docstring says what is kept, for how long and within which bounds.  The words of CAPTURED forwards have owners:
# whoever captures takes a handle (`graph_flags()`), captures inside `with handle:` and calls `handle.release()` when the
# graphs are destroyed; `check_overflow()` reads the words of every live handle, and releasing one leaves the others alone.
# A capture outside any handle lands in one anonymous handle, which only the release-everything teardown below forgets.
_sync_free = {"enabled": False, "headroom": 1.5}
_ledger = StatusLedger()


def set_sync_free(enabled: bool, headroom: float = 1.5):
    _sync_free["enabled"], _sync_free["headroom"] = bool(enabled), float(headroom)


def sync_free_enabled() -> bool:
    return bool(_sync_free["enabled"])


@contextlib.contextmanager
def exact_counts():
    """``with exact_counts():`` forwards inside run on the exact path (capacity mode off); the mode and its headroom are what
    they were afterwards.  For a driver that measures instance counts in the middle of a capacity-mode run."""
    was = dict(_sync_free)
    _sync_free["enabled"] = False
    try:
        yield
    finally:
        _sync_free.update(was)


def reserve_capacity(P: int, W: int, H: int, R: int) -> None:
    """Set the capacity hint of shape ``(P, W, H)`` to ``R`` instances: the next capacity-mode forwards of that shape (a
    hipGraph capture among them) size their binning scratch from it (x headroom).  For a captured iteration that serves
    several cameras: an exact forward overwrites the hint with ITS count, so measure every camera and reserve the maximum."""
    _ledger.remember_hint((int(P), int(W), int(H)), int(R))


def capacity_hint(P: int, W: int, H: int) -> Optional[int]:
    """The capacity hint of shape ``(P, W, H)``: the instance count of its last exact forward, what `reserve_capacity` set or
    what an overflow doubled it to.  None if there is none."""
    return _ledger.hint((int(P), int(W), int(H)))


def forget_capacity(P: int, W: int, H: int) -> None:
    _ledger.forget_hint((int(P), int(W), int(H)))


# MGS_FLAG_EXCLUSIVE_DEVICE (include/monogs_raster.h): the caller vouches that nothing else runs on the device beside the
# forwards issued while this is on -- one process, one stream.  Off by default: MonoGS shares one GPU between three processes.
_call_flags = {"exclusive": False}


@contextlib.contextmanager
def exclusive_device(on: bool = True):
    """``with exclusive_device():`` forwards issued (or captured) inside may assume an otherwise idle device: the small radix
    sorts skip their ticket atomics.  For single-stream loops of a process that owns the GPU (the harness's tracking replays)."""
    prev, _call_flags["exclusive"] = _call_flags["exclusive"], bool(on)
    try:
        yield
    finally:
        _call_flags["exclusive"] = prev


def check_overflow() -> bool:
    """Reads the status words of the forwards issued since the last call, and of every captured forward whose handle is
    live (synchronises).  True if a capacity-mode forward dropped instances -- the capacity hints of the offending shapes
    are doubled, redo the iteration.  Raises if a radix-sort look-back timed out in any forward (exact or capacity mode):
    its blend order, hence its images and gradients, are invalid."""
    return _ledger.check()


def graph_flags() -> GraphFlags:
    """A handle that owns the status words of the forwards captured inside ``with handle:``.  ``handle.release()`` when the
    graphs are destroyed; ``handle.accumulate(sticky)`` for a graph whose replays between two checks must all be seen."""
    return _ledger.graph_flags()


def clear_graph_flags():
    """Teardown for tests and tools: release EVERY handle, the anonymous one of bare ``torch.cuda.graph`` captures included.
    A driver releases its own handle instead."""
    _ledger.release_all()


# ---- optional per-stage timing (bench.py) --------------------------------------------------
_timing_sink: Optional[list] = None


@contextlib.contextmanager
def collect_timing():
    """Within the block every forward/backward appends a dict of per-stage device milliseconds
    (HIP events on the launch stream, see mgs_timing) to the yielded list.  Synchronises."""
    global _timing_sink
    prev, _timing_sink = _timing_sink, []
    try:
        yield _timing_sink
    finally:
        _timing_sink = prev


def _al(n: int) -> int:
    return (int(n) + 255) // 256 * 256


def _camera(rs: GaussianRasterizationSettings, sh_coeffs: int, keep: list, scale_dim: int = 3) -> _lib.MgsCamera:
    cam = _lib.MgsCamera()
    cam.scale_dim = int(scale_dim)
    cam.flags = _lib.FLAG_EXCLUSIVE_DEVICE if _call_flags["exclusive"] else 0
    cam.image_height, cam.image_width = int(rs.image_height), int(rs.image_width)
    cam.tanfovx, cam.tanfovy = float(rs.tanfovx), float(rs.tanfovy)
    cam.scale_modifier = float(rs.scale_modifier)
    cam.sh_degree, cam.sh_coeffs = int(rs.sh_degree), int(sh_coeffs)
    for field in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos"):
        t = _f32(getattr(rs, field).detach(), f"raster_settings.{field}")
        keep.append(t)
        setattr(cam, field, t.data_ptr())
    return cam


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                theta, rho, raster_settings, intr=None):
        lib = _lib.load()
        rs = raster_settings
        means3D = _f32(means3D.detach(), "means3D")
        P = means3D.shape[0]
        dev = means3D.device
        opt = lambda t, n: _f32(t.detach(), n) if (t is not None and t.numel() > 0) else None  # noqa: E731
        sh_ = opt(sh, "shs")
        col_ = opt(colors_precomp, "colors_precomp")
        opac_ = _f32(opacities.detach(), "opacities")
        sc_ = opt(scales, "scales")
        rot_ = opt(rotations, "rotations")
        cov_ = opt(cov3Ds_precomp, "cov3D_precomp")
        M = 0 if sh_ is None else int(sh_.shape[1])
        H, W = int(rs.image_height), int(rs.image_width)

        with _device_guard(dev):
            keep = []
            scale_dim = int(sc_.shape[1]) if sc_ is not None else 3     # [P,1]: isotropic, expanded inside the kernels
            if scale_dim not in (1, 3):
                raise Exception("scales must be [P,3] (or [P,1] for an isotropic map)")
            cam = _camera(rs, M, keep, scale_dim)
            timing = _lib.MgsTiming() if _timing_sink is not None else None
            tref = C.byref(timing) if timing is not None else None
            u8 = dict(dtype=torch.uint8, device=dev)
            # ONE allocation for everything the backward needs back (geometry + image scratch and the scratch of the backward
            # itself), one for the three images and one for the two per-Gaussian integer results: ten torch.empty per forward
            # were ~35 us of host time at SLAM sizes.  LIFETIME: the arena (~250 B per Gaussian + 8 B per pixel) lives as long as
            # the autograd graph of this forward (it is what the backward reads) -- not as long as any OUTPUT: `radii` and
            # `n_touched` are views of their own 8 P-byte tensor, which a caller may keep (WindowMapper does, per keyframe;
            # MonoGS keeps `radii` in render_pkg) without pinning the scratch.  The three images share one 20 HW-byte tensor.
            want_bwd = P > 0 and any(ctx.needs_input_grad)
            n_geom, n_img = _al(lib.mgs_geometry_bytes(P)), _al(lib.mgs_image_bytes(W, H))
            n_bwd = _al(lib.mgs_backward_bytes(P)) if want_bwd else 0
            arena = torch.empty(n_geom + n_img + n_bwd + 256, **u8)
            base = arena.data_ptr()
            off0 = (-base) % 256                                    # the carving functions expect 256-byte-aligned bases
            geom_p, img_p = base + off0, base + off0 + n_geom
            o_r = off0 + n_geom + n_img
            ri = torch.empty(2, P, dtype=torch.int32, device=dev)
            radii, n_touched = ri[0], ri[1]
            # The scratch of the backward that will follow is handed to the forward: its per-Gaussian kernel clears the
            # gradient lines of the visible Gaussians (and the pose part) on the way, and the backward starts with no
            # clearing launch and no 64 B x P fill.
            ctx.scratch = arena[o_r:o_r + n_bwd] if want_bwd else None
            bwd_p = base + o_r if want_bwd else None
            ctx.scratch_used = False
            out5 = torch.empty(5, H, W, dtype=torch.float32, device=dev)
            color, depth, opacity = out5[0:3], out5[3:4], out5[4:5]
            # The blend backward walks every pixel list from both ends when it is given the finished colour and depth images.
            # They are outputs: held by a weak reference (a strong one would be a cycle through grad_fn, and save_for_backward
            # would turn a caller's in-place edit of an output into an error).  A caller that dropped or edited them gets the
            # walk from the back only -- same gradients to rounding.
            ctx.out_ref = weakref.ref(out5) if want_bwd else None
            status = torch.empty(1, dtype=torch.int32, device=dev) if P > 0 else None      # this forward's MGS_STATUS_* word
            key = (P, W, H)
            capturing = torch.cuda.is_current_stream_capturing()
            hint = _ledger.hint(key)
            if capturing and hint is None:
                raise RuntimeError("graph capture needs a capacity hint: run one eager forward with the same "
                                   "(P, W, H) first")
            if not capturing:
                _ledger.raise_failures()
            if (capturing or _sync_free["enabled"]) and hint is not None and P > 0:
                # ---- capacity mode: no read-back, no stream sync, one crossing of the FFI boundary
                R = max(int(hint * _sync_free["headroom"]) + 4096, 4096)
                binning = torch.empty(lib.mgs_binning_bytes(R, W, H), **u8)
                _lib.check(lib.mgs_forward_capacity(
                    C.byref(cam), P, _ptr(means3D), _ptr(sh_), _ptr(col_), _ptr(opac_), _ptr(sc_), _ptr(rot_), _ptr(cov_),
                    geom_p, radii.data_ptr(), bwd_p, R, binning.data_ptr(), img_p, color.data_ptr(), depth.data_ptr(),
                    opacity.data_ptr(), n_touched.data_ptr(), status.data_ptr(), tref, _stream()), "mgs_forward_capacity")
                _ledger.record_capacity(key, status, capturing)
                ctx.overflow = status
            else:
                num_rendered, prev_bits = C.c_uint64(0), C.c_uint32(0)
                here = (torch._C._cuda_getDevice(), _stream())
                prev = _ledger.exact_rider(*here)           # the previous exact forward's word, if it ran on this stream
                _lib.check(lib.mgs_forward_preprocess(
                    C.byref(cam), P, _ptr(means3D), _ptr(sh_), _ptr(col_), _ptr(opac_), _ptr(sc_), _ptr(rot_),
                    _ptr(cov_), geom_p, radii.data_ptr(), bwd_p, C.byref(num_rendered),
                    prev.data_ptr() if prev is not None else None, C.byref(prev_bits) if prev is not None else None,
                    tref, _stream()), "mgs_forward_preprocess")
                _ledger.exact_rider_read(prev_bits.value)   # the PREVIOUS exact forward's sort timed out: raised here
                R = int(num_rendered.value)
                _ledger.remember_hint(key, R)
                binning = torch.empty(lib.mgs_binning_bytes(R, W, H), **u8)
                _lib.check(lib.mgs_forward_render(
                    C.byref(cam), P, R, geom_p, binning.data_ptr(), img_p, color.data_ptr(),
                    depth.data_ptr(), opacity.data_ptr(), n_touched.data_ptr(), _ptr(status), tref, _stream()),
                    "mgs_forward_render")
                if status is not None:      # (the depth sort's flag was already checked at the count read-back)
                    _ledger.record_exact(key, status, *here)
                ctx.overflow = None
            if rs.debug:                    # upstream's debug flag: synchronise and check right after the forward
                check_overflow()
            if timing is not None:
                d = timing.as_dict()
                d.update(kind="forward", num_rendered=R, P=P)
                _timing_sink.append(d)

        ctx.cam, ctx.keep = cam, keep          # the backward reuses the camera block (and keeps its tensors alive)
        ctx.geom_off, ctx.img_off = off0, off0 + n_geom
        ctx.raster_settings = rs
        ctx.num_rendered = R
        ctx.sh_coeffs = M
        ctx.scale_dim = scale_dim
        ctx.has = (sh_ is not None, col_ is not None, sc_ is not None, cov_ is not None,
                   theta is not None, rho is not None)
        ctx.has_intr = intr is not None
        dummy = torch.empty(0, device=dev)
        ctx.save_for_backward(means3D, sh_ if sh_ is not None else dummy, col_ if col_ is not None else dummy,
                              opac_, sc_ if sc_ is not None else dummy, rot_ if rot_ is not None else dummy,
                              cov_ if cov_ is not None else dummy, radii, arena, binning)
        ctx.out_version = out5._version
        ctx.mark_non_differentiable(radii, n_touched)
        ctx.set_materialize_grads(False)     # unused output gradients arrive as None instead of three zero-fill kernels
        return color, radii, depth, opacity, n_touched

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_opacity, grad_n_touched):
        # grad_opacity is ignored, as upstream does
        lib = _lib.load()
        rs = ctx.raster_settings
        means3D, sh_, col_, opac_, sc_, rot_, cov_, radii, arena, binning = ctx.saved_tensors
        geom_p, img_p = arena.data_ptr() + ctx.geom_off, arena.data_ptr() + ctx.img_off
        has_sh, has_col, has_sr, has_cov, has_theta, has_rho = ctx.has
        P = means3D.shape[0]
        dev = means3D.device
        H, W = int(rs.image_height), int(rs.image_width)
        need = ctx.needs_input_grad   # means3D, means2D, sh, colors, opacities, scales, rotations, cov3D, theta, rho, -, intr
        want_intr = ctx.has_intr and len(need) > 11 and need[11]

        with _device_guard(dev):
            cam = ctx.cam
            f32 = dict(dtype=torch.float32, device=dev)
            g_color = _f32(grad_color, "grad_color") if grad_color is not None else torch.zeros(3, H, W, **f32)
            g_depth = _f32(grad_depth, "grad_depth") if grad_depth is not None else torch.zeros(1, H, W, **f32)
            out = lambda cond, *shape: torch.empty(*shape, **f32) if cond else None  # noqa: E731
            d_means2D = out(need[1], P, 3)
            d_sh = out(need[2] and has_sh, P, max(ctx.sh_coeffs, 1), 3)
            d_cov = out(need[7] and has_cov, P, 6)
            # The gradients of the replicated map parameters (xyz, colour, opacity, scale, rotation) are carved out of ONE
            # allocation, in that order: a keyframe-sharded mapping window can then all-reduce them with a single
            # collective over the flat storage, with no pack / unpack copies (window.GradBucket finds the adjacency).
            widths = [3 if need[0] else 0, 3 if (need[3] and has_col) else 0, 1 if need[4] else 0,
                      ctx.scale_dim if (need[5] and has_sr) else 0, 4 if (need[6] and has_sr) else 0]
            flat = torch.empty(P * sum(widths), **f32) if sum(widths) else None
            views, o = [], 0
            for w in widths:
                views.append(flat[o:o + P * w].view(P, w) if w else None)
                o += P * w
            d_means3D, d_col, d_opac, d_scales, d_rot = views
            want_tau = (need[8] and has_theta) or (need[9] and has_rho) or want_intr
            n_tau = 10 if want_intr else 6      # MGS_FLAG_INTRINSICS_GRAD: (rho, theta, dfx, dfy, dcx, dcy)
            if want_intr:                       # (a copy: the forward's camera block stays as the forward scratch handle saw it)
                cam = _lib.MgsCamera.from_buffer_copy(cam)
                cam.flags |= _lib.FLAG_INTRINSICS_GRAD
            prepared = ctx.scratch is not None and not ctx.scratch_used      # (a second backward through the same forward
            ctx.scratch_used = True                                          #  clears a fresh scratch with a launch)
            scratch = ctx.scratch if prepared else torch.empty(lib.mgs_backward_bytes(P), dtype=torch.uint8, device=dev)
            if want_tau and prepared:       # the six floats live inside the prepared scratch (the forward cleared them)
                off = int(lib.mgs_backward_tau(scratch.data_ptr(), P)) - scratch.data_ptr()
                d_tau = scratch[off:off + 4 * n_tau].view(torch.float32)
            else:
                d_tau = torch.empty(n_tau, **f32) if want_tau else None
            timing = _lib.MgsTiming() if _timing_sink is not None else None
            tref = C.byref(timing) if timing is not None else None
            out5 = ctx.out_ref() if ctx.out_ref is not None else None
            if out5 is not None and out5._version != ctx.out_version:
                out5 = None
            _lib.check(lib.mgs_backward(
                C.byref(cam), P, ctx.num_rendered,
                _ptr(means3D), _ptr(sh_) if has_sh else None, _ptr(col_) if has_col else None, _ptr(opac_),
                _ptr(sc_) if has_sr else None, _ptr(rot_) if has_sr else None, _ptr(cov_) if has_cov else None,
                radii.data_ptr(), geom_p, binning.data_ptr(), img_p,
                g_color.data_ptr(), g_depth.data_ptr(),
                out5.data_ptr() if out5 is not None else None,                 # colour [3,H,W], depth [1,H,W] behind it
                out5.data_ptr() + 12 * H * W if out5 is not None else None,
                _ptr(d_means2D), _ptr(d_col), _ptr(d_opac), _ptr(d_means3D), _ptr(d_cov), _ptr(d_sh),
                _ptr(d_scales), _ptr(d_rot), _ptr(d_tau), scratch.data_ptr(), 1 if prepared else 0, tref, _stream()),
                "mgs_backward")
            if timing is not None:
                d = timing.as_dict()
                d.update(kind="backward", num_rendered=ctx.num_rendered, P=P)
                _timing_sink.append(d)
        # (views of the 6-float result: autograd takes them as .grad without a copy kernel)
        d_theta = d_tau[3:6] if (d_tau is not None and need[8] and has_theta) else None
        d_rho = d_tau[:3] if (d_tau is not None and need[9] and has_rho) else None
        if not ctx.has_intr:
            return (d_means3D, d_means2D, d_sh, d_col, d_opac, d_scales, d_rot, d_cov, d_theta, d_rho, None)
        return (d_means3D, d_means2D, d_sh, d_col, d_opac, d_scales, d_rot, d_cov, d_theta, d_rho, None,
                d_tau[6:10] if want_intr else None)


class ForwardScratch(NamedTuple):
    """What a finished forward left behind for whoever reads its lists afterwards (the feature kernels, the viewer's ellipsoid
    walk, the blend statistics).  Strong references: they outlive the rasteriser's own backward, which frees its saved tensors,
    for as long as the colour image (its ``grad_fn``) or anything rendered from the handle lives."""
    cam: object                 # _lib.MgsCamera of the forward
    keep: list                  # the tensors its pointers name
    arena: torch.Tensor         # geometry + image scratch
    binning: torch.Tensor
    geom_off: int
    img_off: int
    num_rendered: int           # the capacity, after a capacity-mode forward
    P: int
    H: int
    W: int
    device: torch.device

    def pointers(self):
        """``(geometry, binning, image)`` as the C ABI takes them."""
        base = self.arena.data_ptr()
        return base + self.geom_off, self.binning.data_ptr(), base + self.img_off


def forward_scratch(color: torch.Tensor, who: str = "forward_scratch") -> ForwardScratch:
    """The handle of the forward that produced ``color``.  Built on the first request and kept on the autograd node, so the
    forward itself does nothing for it; ask once before the rasteriser's backward to read the scratch after it."""
    fn = getattr(color, "grad_fn", None)
    if fn is None or not hasattr(fn, "raster_settings"):
        raise RuntimeError(f"{who} needs the colour image of a differentiable rasteriser forward")
    t = getattr(fn, "_forward_scratch", None)
    if t is None:
        try:
            means3D, _, _, _, _, _, _, _, arena, binning = fn.saved_tensors
        except RuntimeError as e:
            raise RuntimeError(f"{who}: the rasteriser's backward has already freed this forward's scratch; "
                               f"call {who} once before that backward to keep it") from e
        rs = fn.raster_settings
        t = ForwardScratch(fn.cam, fn.keep, arena, binning, int(fn.geom_off), int(fn.img_off), int(fn.num_rendered),
                           int(means3D.shape[0]), int(rs.image_height), int(rs.image_width), means3D.device)
        fn._forward_scratch = t
    return t


def _blend_counters(color, symbol: str, words: int) -> list:
    t = forward_scratch(color, symbol[4:])
    out = torch.zeros(words, dtype=torch.int64, device=t.device)
    with _device_guard(t.device):
        _lib.check(getattr(_lib.load(), symbol)(C.byref(t.cam), t.P, t.num_rendered, *t.pointers(), out.data_ptr(), _stream()),
                   symbol)
    return out.tolist()


def debug_blend_stats(color: torch.Tensor) -> dict:
    """Diagnostic: what the blend backward of the forward that produced ``color`` walks, fetches and reduces
    (``mgs_debug_blend_stats``; call before ``backward()`` frees the saved scratch).  Synchronises."""
    v = _blend_counters(color, "mgs_debug_blend_stats", _lib.H.MGS_BLEND_STATS_WORDS)
    groups = {}
    for d, name in enumerate(("halves_8x4", "halves_4x8", "blocks_4x4", "strips_8x2", "blocks_4x2")):
        groups[name] = dict(trips_paired_per_step=v[8 + 3 * d], rows=v[9 + 3 * d], trips_own_lists=v[10 + 3 * d])
    return dict(steps=v[0], survivors=v[1], active_survivors=v[2], active_pairs=v[3], inactive_by_depth_order=v[4],
                active_le2=v[5], active_le4=v[6], active_le8=v[7], group_streams=groups)


def debug_blend_mask_stats(color: torch.Tensor) -> dict:
    """Diagnostic: the survivor masks the blend forward that produced ``color`` left for its backward, against the cull the
    backward would run for itself (``mgs_debug_blend_mask_stats``; call before ``backward()`` frees the saved scratch).
    Synchronises."""
    v = _blend_counters(color, "mgs_debug_blend_mask_stats", _lib.H.MGS_BLEND_MASK_STATS_WORDS)
    return dict(steps=v[0], own_cull=v[1], forward_masks=v[2], missing=v[3])


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        theta, rho, raster_settings, intr=None):
    if intr is None:        # today's call, argument for argument
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                         cov3Ds_precomp, theta, rho, raster_settings)
    if tuple(intr.shape) != (4,) or intr.dtype != torch.float32 or intr.device != means3D.device:
        raise RuntimeError("intr must be a [4] float32 tensor (fx, fy, cx, cy) on the device of means3D")
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, theta, rho, raster_settings, intr)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """bool[P]: inside the view frustum's near side (view-space z > 0.2)."""
        lib = _lib.load()
        rs = self.raster_settings
        with torch.no_grad():
            pos = _f32(positions, "positions")
            P = pos.shape[0]
            vis = torch.zeros(P, dtype=torch.uint8, device=pos.device)
            with _device_guard(pos.device):
                vm = _f32(rs.viewmatrix, "viewmatrix")
                pm = _f32(rs.projmatrix, "projmatrix")
                _lib.check(lib.mgs_mark_visible(P, pos.data_ptr(), vm.data_ptr(), pm.data_ptr(), vis.data_ptr(),
                                                _stream()), "mgs_mark_visible")
        return vis.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, theta=None, rho=None):
        # (the reference's signature, parameter for parameter -- tests/test_host_api.py holds the drop-in packages to it; the one
        #  keyword the reference does not have, ``intr``, is taken by ``__call__`` below, which is how every caller calls the module)
        return self._rasterize(means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, theta, rho)

    def __call__(self, *args, intr=None, **kwargs):
        """``rasterizer(means3D=..., ..., theta=None, rho=None, intr=None)``: ``forward`` plus ``intr``.  ``theta``, ``rho`` and
        ``intr`` are delta holders: their values are not read (they are zero at call time); they exist to receive ``.grad`` --
        dL/dtheta, dL/drho and, for ``intr`` ([4] float32), dL/d(fx, fy, cx, cy) in pixels, evaluated at the intrinsics the raster
        settings were built from (``MGS_FLAG_INTRINSICS_GRAD``).  Without ``intr`` this is ``nn.Module.__call__``."""
        if intr is None:
            return super().__call__(*args, **kwargs)
        return self._rasterize(*args, intr=intr, **kwargs)

    def _rasterize(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                   cov3D_precomp=None, theta=None, rho=None, intr=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, theta, rho, rs, intr)
