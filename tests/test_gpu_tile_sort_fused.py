"""The per-tile depth sort folded into the blend forward (option "tile_sort_fused" = 1, the default) against the same sort
as a launch of its own (= 0): the same tables and images bit for bit, on scenes forced onto the per-tile path
(radix_scanned = 1).  The cases are those of test_gpu_tile_depth_sort.py: ties, far depths, long lists, capacity overflow."""
import ctypes as C

import pytest
import torch

from monogs_amd.synthetic import make_scene, scene_settings

DEV = "cuda:0"
KEYS = ("point_list", "ranges", "color", "depth", "opacity", "final_T", "n_contrib", "n_touched", "radii")


def _settings(sc):
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    return scene_settings(sc, GaussianRasterizationSettings, device=DEV)


def _args(sc):
    return dict(colors_precomp=sc.colors.to(DEV), scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV))


class _opts:
    """Per-tile path, sort fused or not, for the duration of a block (the options are process-global)."""

    def __init__(self, lib, fused):
        self.lib, self.fused = lib, fused

    def __enter__(self):
        assert self.lib.mgs_debug_set_option(b"radix_scanned", 1) == 0
        assert self.lib.mgs_debug_set_option(b"tile_sort_fused", self.fused) == 0

    def __exit__(self, *exc):
        self.lib.mgs_debug_set_option(b"radix_scanned", -1)
        self.lib.mgs_debug_set_option(b"tile_sort_fused", -1)


def _tables(lib, sc, fused):
    from monogs_amd.debug import forward_tables
    with _opts(lib, fused):
        t = forward_tables(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc))
    assert t["depth_path"] == "per_tile" and t["status"] == 0
    return t


def _grads(lib, sc, fused):
    from monogs_amd.rasterizer import GaussianRasterizer
    with _opts(lib, fused):
        leaves = {k: v.to(DEV).clone().requires_grad_(True) for k, v in
                  dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors,
                       scales=sc.scales.repeat(1, 3), rotations=sc.rotations).items()}
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        theta = torch.zeros(3, device=DEV, requires_grad=True)
        rho = torch.zeros(3, device=DEV, requires_grad=True)
        color, radii, depth, opacity, n_touched = GaussianRasterizer(_settings(sc))(
            means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
            colors_precomp=leaves["colors_precomp"], scales=leaves["scales"], rotations=leaves["rotations"],
            theta=theta, rho=rho)
        loss = (color * sc.grad_color.to(DEV)).sum() + (depth * sc.grad_depth.to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
    g = {k: v.grad.detach().cpu() for k, v in leaves.items()}
    g.update(means2D=means2D.grad.cpu(), theta=theta.grad.cpu(), rho=rho.grad.cpu(), color=color.detach().cpu(),
             depth=depth.detach().cpu(), n_touched=n_touched.cpu())
    return g


def _check(lib, sc):
    a, b = _tables(lib, sc, 1), _tables(lib, sc, 0)
    assert a["num_rendered"] == b["num_rendered"]
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    # The backward reads the same ranges and point list; its float atomics may add in another order from run to run.  On
    # the long-list scene two runs of one path differ by up to 2.5e-6 max|ref|, so the bound is test_gpu_parity.py's
    # absolute floor, 1e-5 max|ref|, with float32 round-off (1e-5) relative to each element.
    ga, gb = _grads(lib, sc, 1), _grads(lib, sc, 0)
    for k in ("color", "depth", "n_touched"):
        assert torch.equal(ga[k], gb[k]), k
    for k, ref in gb.items():
        scale = ref.abs().max().item()
        assert torch.allclose(ga[k].float(), ref.float(), rtol=1e-5, atol=1e-5 * max(scale, 1e-30)), k
    return a


def test_tile_sort_fused_option_is_known(native_lib):
    """Host-only: the option exists, takes 0 / 1, and -1 restores the default."""
    for v in (0, 1, -1):
        assert native_lib.mgs_debug_set_option(b"tile_sort_fused", v) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("P,intr,seed", [(5000, "fr3_office", 0), (20000, "replica", 7)])
def test_fused_matches_the_separate_launch(native_lib, P, intr, seed):
    _check(native_lib, make_scene(P, intr, seed=seed))


@pytest.mark.gpu
def test_fused_exact_depth_ties(native_lib):
    sc = make_scene(8000, "fr3_office", seed=3)
    f = lambda t: t.clone()  # noqa: E731
    means, scales, rots, opac, cols = f(sc.means3D), f(sc.scales), f(sc.rotations), f(sc.opacities), f(sc.colors)
    for t in (means, scales, rots, opac, cols):                     # every 7th Gaussian repeats the one before it
        t[7::7] = t[6:-1:7][: t[7::7].shape[0]]
    _check(native_lib, sc._replace(means3D=means, scales=scales, rotations=rots, opacities=opac, colors=cols))


@pytest.mark.gpu
def test_fused_depths_beyond_the_narrow_range(native_lib):
    K = 4000.0
    sc = make_scene(20000, "fr3_office", seed=11, near_fraction=0.0)
    sc = sc._replace(means3D=sc.means3D * K, scales=sc.scales * K, t=sc.t * K)
    a = _check(native_lib, sc)
    depth = a["rec"][:, 11]
    vis = a["radii"] > 0
    assert float(depth[vis].max()) > 13107.2 > float(depth[vis].min())


@pytest.mark.gpu
def test_fused_lists_longer_than_the_lds(native_lib):
    """Tiles of more than 1024 pairs are sorted in global memory and walked from point_list, the others from LDS."""
    a = _check(native_lib, make_scene(12000, "fr3_office", seed=4, mean_radius_px=80.0))
    n = (a["ranges"][:, 1] - a["ranges"][:, 0]).long()
    assert int((n > 1024).sum()) > 0 and int(((n > 0) & (n <= 1024)).sum()) > 0


def _au(v, a=256):
    return (v + a - 1) // a * a


@pytest.mark.gpu
def test_fused_capacity_below_the_instance_count(native_lib):
    """Capacity mode with half the slots: the same overflow word, images, ranges and live point list either way."""
    from monogs_amd import _lib
    from monogs_amd.rasterizer import _camera, _f32, _ptr, _stream
    lib = native_lib
    sc = make_scene(20000, "replica", seed=2)
    st = _settings(sc)
    H, W, P = int(st.image_height), int(st.image_width), sc.means3D.shape[0]
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    tile_bits = max(1, (ntiles - 1).bit_length())
    args = _args(sc)
    means, opac = _f32(sc.means3D.to(DEV), "means3D"), _f32(sc.opacities.to(DEV), "opacities")
    cols, scales, rots = _f32(args["colors_precomp"], "c"), _f32(args["scales"], "s"), _f32(args["rotations"], "r")
    out = {}
    for fused in (1, 0):
        with _opts(lib, fused):
            keep = []
            cam = _camera(st, 0, keep, 3)
            u8 = dict(dtype=torch.uint8, device=DEV)
            geom = torch.zeros(lib.mgs_geometry_bytes(P), **u8)
            img = torch.zeros(lib.mgs_image_bytes(W, H), **u8)
            radii = torch.empty(P, dtype=torch.int32, device=DEV)
            n_touched = torch.empty(P, dtype=torch.int32, device=DEV)
            o = [torch.empty(c, H, W, dtype=torch.float32, device=DEV) for c in (3, 1, 1)]
            nr = C.c_uint64(0)
            _lib.check(lib.mgs_forward_preprocess(C.byref(cam), P, _ptr(means), None, _ptr(cols), _ptr(opac), _ptr(scales),
                                                  _ptr(rots), None, geom.data_ptr(), radii.data_ptr(), None, C.byref(nr),
                                                  None, None, None, _stream()), "preprocess")
            R = int(nr.value)
            cap = R // 2
            binning = torch.zeros(lib.mgs_binning_bytes(cap, W, H), **u8)
            over = torch.zeros(1, dtype=torch.int32, device=DEV)
            _lib.check(lib.mgs_forward_render_capacity(C.byref(cam), P, cap, geom.data_ptr(), binning.data_ptr(),
                                                       img.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                       n_touched.data_ptr(), over.data_ptr(), None, _stream()),
                       "render_capacity")
            torch.cuda.synchronize()
            assert lib.mgs_binning_path(P, W, H) == 1

            def view(buf, off, nbytes, dtype):
                base = _au(buf.data_ptr()) - buf.data_ptr()
                return buf[base + off: base + off + nbytes].view(dtype)

            ranges = view(img, 2 * _au(H * W * 4), ntiles * 8, torch.int32).reshape(ntiles, 2).clone()
            in_b = ((tile_bits + 7) // 8) % 2 == 1
            point_list = view(binning, (3 if in_b else 2) * _au(cap * 4), cap * 4, torch.int32)
            live = int(ranges[:, 1].max())
            out[fused] = dict(over=int(over.item()), R=R, color=o[0].clone(), depth=o[1].clone(), opacity=o[2].clone(),
                              n_touched=n_touched.clone(), ranges=ranges, live=live, point_list=point_list[:live].clone(),
                              final_T=view(img, 0, H * W * 4, torch.float32).clone(),
                              n_contrib=view(img, _au(H * W * 4), H * W * 4, torch.int32).clone())
    a, b = out[1], out[0]
    assert a["over"] != 0 and a["over"] == b["over"] and a["R"] == b["R"]
    assert 0 < a["live"] <= a["R"] // 2
    for k in ("color", "depth", "opacity", "n_touched", "ranges", "point_list", "final_T", "n_contrib"):
        assert torch.equal(a[k], b[k]), k
