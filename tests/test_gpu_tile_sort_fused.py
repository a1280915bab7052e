"""The per-tile depth sort folded into the blend forward (option "tile_sort_fused" = 1, the default) against the same sort
as a launch of its own (= 0): the same tables and images bit for bit, on scenes forced onto the per-tile path
(radix_scanned = 1).  The cases are those of test_gpu_tile_depth_sort.py: ties, far depths, long lists, capacity overflow."""
import pytest
import torch

from monogs_amd.debug import options
from monogs_amd.synthetic import make_scene, scene_settings

DEV = "cuda:0"
KEYS = ("point_list", "ranges", "color", "depth", "opacity", "final_T", "n_contrib", "n_touched", "radii")


def _settings(sc):
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    return scene_settings(sc, GaussianRasterizationSettings, device=DEV)


def _args(sc):
    return dict(colors_precomp=sc.colors.to(DEV), scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV))


def _tables(lib, sc, fused):
    from monogs_amd.debug import forward_tables
    with options(radix_scanned=1, tile_sort_fused=fused):
        t = forward_tables(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc))
    assert t["depth_path"] == "per_tile" and t["status"] == 0
    return t


def _grads(lib, sc, fused):
    from monogs_amd.rasterizer import GaussianRasterizer
    with options(radix_scanned=1, tile_sort_fused=fused):
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


@pytest.mark.gpu
def test_fused_capacity_below_the_instance_count(native_lib):
    """Capacity mode with half the slots: the same overflow word, images, ranges and live point list either way."""
    from monogs_amd.debug import RawForward
    sc = make_scene(20000, "replica", seed=2)
    out = {}
    for fused in (1, 0):
        with options(radix_scanned=1, tile_sort_fused=fused):
            f = RawForward(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc), zero=True)
            R = f.preprocess()
            f.render(R // 2, capacity=True)
            assert native_lib.mgs_binning_path(f.P, f.W, f.H) == 1
            ranges = f.table("image.ranges").reshape(-1, 2).clone()
            live = int(ranges[:, 1].max())
            out[fused] = dict(over=int(f.status.item()), R=R, color=f.color.clone(), depth=f.depth.clone(),
                              opacity=f.opacity.clone(), n_touched=f.n_touched.clone(), ranges=ranges, live=live,
                              point_list=f.table("binning.point_list")[:live].clone(),
                              final_T=f.table("image.final_T").clone(), n_contrib=f.table("image.n_contrib").clone())
    a, b = out[1], out[0]
    assert a["over"] != 0 and a["over"] == b["over"] and a["R"] == b["R"]
    assert 0 < a["live"] <= a["R"] // 2
    for k in ("color", "depth", "opacity", "n_touched", "ranges", "point_list", "final_T", "n_contrib"):
        assert torch.equal(a[k], b[k]), k
