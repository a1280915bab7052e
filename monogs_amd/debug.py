"""Test/diagnostic access to the rasteriser below its autograd wrapper: the process-global test knobs for the duration of a
block (``options``), the raw C ABI forward and backward on one scene's buffers (``RawForward``) and the binning tables a
forward leaves in its scratch (``forward_tables``).  Where a sub-buffer lies is asked of the library
(``mgs_debug_scratch_field``, include/monogs_raster.h): nothing here computes an offset."""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import _lib
from ._launch import _f32, _ptr, _stream, _device_guard
from .rasterizer import _camera

_FLOAT_TABLES = ("geometry.rec", "image.final_T", "backward.grad_acc", "backward.tau_part", "backward.tau")


@contextlib.contextmanager
def options(**knobs):
    """``with options(radix_scanned=1, pre_scan=0):`` -- ``mgs_debug_set_option`` for the duration of a block, every knob back
    at its default (-1) afterwards.  The knobs are process-global: not for use beside other threads inside the library."""
    lib = _lib.load()
    done = []
    try:
        for name, value in knobs.items():
            _lib.check(lib.mgs_debug_set_option(name.encode(), int(value)), "mgs_debug_set_option")
            done.append(name)
        yield
    finally:
        for name in reversed(done):
            lib.mgs_debug_set_option(name.encode(), -1)


class RawForward:
    """One scene's buffers and the raw calls on them: ``preprocess`` (optionally handing over the backward's scratch),
    ``render`` (exact or capacity mode), ``backward``; ``table(name)`` views a sub-buffer of the four scratches afterwards.
    The binning scratch is ``torch.empty`` (the library must not rely on a cleared one); geometry and image scratch are
    zero-filled with ``zero=True``.  ``grad_color`` / ``grad_depth`` are needed by ``backward`` only."""

    def __init__(self, rs, means3D, opacities, colors_precomp=None, shs=None, scales=None, rotations=None, cov3D_precomp=None,
                 grad_color=None, grad_depth=None, zero=False):
        self.lib = lib = _lib.load()
        self.device = dev = means3D.device
        self.P = P = means3D.shape[0]
        self.H, self.W = H, W = int(rs.image_height), int(rs.image_width)
        c = lambda t, n: None if t is None else _f32(t.detach(), n)  # noqa: E731
        self.means, self.opac = c(means3D, "means3D"), c(opacities, "opacities")
        self.col, self.shs, self.scales = c(colors_precomp, "colors"), c(shs, "shs"), c(scales, "scales")
        self.rot, self.cov = c(rotations, "rotations"), c(cov3D_precomp, "cov3D")
        self.g_color, self.g_depth = c(grad_color, "grad_color"), c(grad_depth, "grad_depth")
        scale_dim = int(self.scales.shape[1]) if self.scales is not None else 3       # [P,1]: isotropic, expanded inside the kernels
        if scale_dim not in (1, 3):
            raise Exception("scales must be [P,3] (or [P,1] for an isotropic map)")
        self.keep = []
        with _device_guard(dev):
            self.cam = _camera(rs, 0 if self.shs is None else self.shs.shape[1], self.keep, scale_dim)
            u8 = dict(dtype=torch.uint8, device=dev)
            alloc = torch.zeros if zero else torch.empty
            self.geom = alloc(lib.mgs_geometry_bytes(P), **u8)
            self.img = alloc(lib.mgs_image_bytes(W, H), **u8)
            self.scratch = torch.empty(lib.mgs_backward_bytes(P), **u8)
            self.radii = torch.empty(P, dtype=torch.int32, device=dev)
            self.n_touched = torch.empty(P, dtype=torch.int32, device=dev)
            self.out = torch.empty(5, H, W, dtype=torch.float32, device=dev)
            self.color, self.depth, self.opacity = self.out[0:3], self.out[3:4], self.out[4:5]
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.binning, self.R = None, 0

    def _inputs(self):
        return [_ptr(t) for t in (self.means, self.shs, self.col, self.opac, self.scales, self.rot, self.cov)]

    def preprocess(self, prepare=False) -> int:
        """``mgs_forward_preprocess`` -> the instance count; ``prepare``: tell it of the backward that will use ``scratch``."""
        nr = C.c_uint64(0)
        with _device_guard(self.device):
            _lib.check(self.lib.mgs_forward_preprocess(
                C.byref(self.cam), self.P, *self._inputs(), self.geom.data_ptr(), self.radii.data_ptr(),
                self.scratch.data_ptr() if prepare else None, C.byref(nr), None, None, None, _stream()), "mgs_forward_preprocess")
        return int(nr.value)

    def render(self, R, capacity=False):
        """``mgs_forward_render`` of ``R`` instances, or ``mgs_forward_render_capacity`` with room for ``R``.  Synchronises."""
        with _device_guard(self.device):
            self.binning = torch.empty(self.lib.mgs_binning_bytes(R, self.W, self.H), dtype=torch.uint8, device=self.device)
            self.R = R
            fn = self.lib.mgs_forward_render_capacity if capacity else self.lib.mgs_forward_render
            _lib.check(fn(C.byref(self.cam), self.P, R, self.geom.data_ptr(), self.binning.data_ptr(), self.img.data_ptr(),
                          self.color.data_ptr(), self.depth.data_ptr(), self.opacity.data_ptr(), self.n_touched.data_ptr(),
                          self.status.data_ptr() if self.P > 0 else None, None, _stream()),
                       "mgs_forward_render_capacity" if capacity else "mgs_forward_render")
            torch.cuda.synchronize()

    def backward(self, prepared) -> dict:
        """``mgs_backward`` into fresh gradient tensors; ``tau`` is read from the six floats inside ``scratch``.  Synchronises."""
        P, f32 = self.P, dict(dtype=torch.float32, device=self.device)
        new = lambda cond, *shape: torch.empty(*shape, **f32) if cond else None  # noqa: E731
        sr = self.scales is not None
        g = dict(means2D=new(True, P, 3), colors=new(self.col is not None, P, 3), opacities=new(True, P, 1),
                 means3D=new(True, P, 3), cov3D=new(self.cov is not None, P, 6),
                 shs=new(self.shs is not None, P, 1 if self.shs is None else self.shs.shape[1], 3),
                 scales=new(sr, P, self.scales.shape[1] if sr else 3), rotations=new(sr, P, 4))
        tau = self.table("backward.tau")[:6]
        with _device_guard(self.device):
            _lib.check(self.lib.mgs_backward(
                C.byref(self.cam), P, self.R, *self._inputs(), self.radii.data_ptr(), self.geom.data_ptr(),
                _ptr(self.binning), self.img.data_ptr(), self.g_color.data_ptr(), self.g_depth.data_ptr(),
                self.color.data_ptr(), self.depth.data_ptr(), *[_ptr(g[k]) for k in g], tau.data_ptr(),
                self.scratch.data_ptr(), 1 if prepared else 0, None, _stream()), "mgs_backward")
            torch.cuda.synchronize()
        g = {k: v for k, v in g.items() if v is not None}
        g["tau"] = tau.clone()
        return g

    def table(self, name, dtype=None):
        """The sub-buffer ``"<scratch>.<member>"`` (``mgs_debug_scratch_field``) as a flat view: float32 for the float tables,
        int32 otherwise, or ``dtype``.  Binning tables are those of the last ``render``."""
        buf = dict(geometry=self.geom, image=self.img, binning=self.binning, backward=self.scratch)[name.split(".")[0]]
        off, n = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.lib.mgs_debug_scratch_field(name.encode(), self.P, self.R, self.W, self.H, C.byref(off), C.byref(n)),
                   "mgs_debug_scratch_field")
        start = (-buf.data_ptr()) % 256 + off.value           # (the carving starts at the next multiple of 256)
        return buf[start:start + n.value].view(dtype or (torch.float32 if name in _FLOAT_TABLES else torch.int32))


def forward_tables(rs, means3D, opacities, colors_precomp=None, shs=None, scales=None, rotations=None,
                   cov3D_precomp=None, between=None):
    """Run the HIP forward and return outputs plus the per-tile tables as torch tensors.  ``between``: called after the
    first stage (per-Gaussian kernel, depth sort, scan) has finished and before the second (duplicate, tile sort, blend) starts.

    ``depth_path`` tells which depth order the forward built (``mgs_binning_path``): "global" (a depth sort of all
    Gaussians, whose result ``perm`` is read from the scratch) or "per_tile" (each tile's list sorted by depth on its own).
    On the per-tile path no kernel materialises ``perm``: it is derived here from the depth keys, in the order the global
    sort defines -- visible Gaussians by (depth key, index), culled ones (key of all ones) last, by index."""
    f = RawForward(rs, means3D, opacities, colors_precomp, shs, scales, rotations, cov3D_precomp, zero=True)
    P, H, W = f.P, f.H, f.W
    per_tile = f.lib.mgs_binning_path(P, W, H) == 1
    R = f.preprocess()
    if between is not None:
        between()
    f.render(R)
    ranges = f.table("image.ranges").reshape(-1, 2)
    ntiles = ranges.shape[0]
    # tile id per sorted instance.  Since round 4 the tile sort's final pass writes the per-tile ranges instead of the sorted
    # keys (nobody reads them): the tile of instance i is the tile whose range holds i.
    rg = ranges.long()
    tile_sorted = torch.repeat_interleave(torch.arange(ntiles, device=ranges.device), (rg[:, 1] - rg[:, 0]).clamp_min(0)).to(torch.int32)
    rec = f.table("geometry.rec").reshape(P, 16)
    if per_tile:
        # rect {x0 | y0 << 16, w | h << 16} by Gaussian index (what the scan and duplicate read); perm from the depth keys
        keys = f.table("geometry.depth_key").long() & 0xFFFFFFFF
        perm = torch.sort(keys, stable=True).indices.to(torch.int32)
        wh = f.table("geometry.rect").reshape(P, 2)[:, 1]
        tiles_touched = (wh & 0xFFFF) * ((wh >> 16) & 0xFFFF)
    else:
        perm = f.table("geometry.perm")
        wh_sorted = f.table("geometry.rect_sorted").reshape(P, 2)[:, 1]
        tiles_touched = torch.zeros(P, dtype=torch.int32, device=f.device)
        # tiles each Gaussian touches = w * h of its rectangle (scattered back from depth order to Gaussian index)
        tiles_touched[perm.long()] = (wh_sorted & 0xFFFF) * ((wh_sorted >> 16) & 0xFFFF)
    depth_key = rec[:, 11].contiguous().view(torch.int32)          # float32 bits of the view-space depth
    return dict(color=f.color, depth=f.depth, opacity=f.opacity, radii=f.radii, n_touched=f.n_touched, num_rendered=R,
                status=int(f.status.item()),
                final_T=f.table("image.final_T").reshape(H, W), n_contrib=f.table("image.n_contrib").reshape(H, W),
                ranges=ranges, tile_sorted=tile_sorted, point_list=f.table("binning.point_list"), rec=rec,
                tiles_touched=tiles_touched, depth_key=depth_key, perm=perm, depth_path="per_tile" if per_tile else "global")
