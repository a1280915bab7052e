"""Per-tile depth order (mgs_binning_path == 1) against the global depth sort (== 0): the same tile lists bit for bit.

Large maps no longer sort all Gaussians by depth: the instances are emitted in index order with their depth bits packed
into the tile sort's pairs, and one workgroup per tile sorts its list by (depth bits, index) in LDS
(csrc/binning.hip, tile_depth_sort_kernel).  The "radix_scanned" option forces either path at any size (1: per tile,
0: the global sort), so small scenes exercise both and compare them."""
import pytest
import torch

from monogs_amd.debug import options
from monogs_amd.synthetic import make_scene, scene_settings

DEV = "cuda:0"


def _settings(sc):
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    return scene_settings(sc, GaussianRasterizationSettings, device=DEV)


def _args(sc):
    return dict(colors_precomp=sc.colors.to(DEV), scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV))


def _tables(lib, sc, value):
    from monogs_amd.debug import forward_tables
    with options(radix_scanned=value):
        return forward_tables(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc))


def _grads(lib, sc, value):
    from monogs_amd.rasterizer import GaussianRasterizer
    with options(radix_scanned=value):
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
    g.update(means2D=means2D.grad.cpu(), theta=theta.grad.cpu(), rho=rho.grad.cpu(), color=color.detach().cpu())
    return g


def _same_tables(a, b):
    assert a["depth_path"] == "per_tile" and b["depth_path"] == "global"
    assert a["status"] == 0 and b["status"] == 0
    assert a["num_rendered"] == b["num_rendered"]
    for k in ("point_list", "ranges", "color", "depth", "opacity", "n_contrib", "n_touched", "final_T", "radii",
              "tiles_touched", "perm"):
        assert torch.equal(a[k], b[k]), k
    # the contract itself: inside every tile, (depth bits, index) strictly increasing
    pl = a["point_list"].long()
    key = (a["tile_sorted"].long() << 32) | (a["depth_key"].long() & 0xFFFFFFFF)[pl]
    d = key[1:] - key[:-1]
    assert bool((d >= 0).all()) and bool((pl[1:][d == 0] > pl[:-1][d == 0]).all())


def _same_grads(lib, sc):
    """The backward reads only the ranges and the point list, which are identical; its float atomics may still add in a
    different order from run to run, so the gradients are held to float32 round-off, not to bits."""
    a, b = _grads(lib, sc, 1), _grads(lib, sc, 0)
    assert torch.equal(a["color"], b["color"])
    for k, ref in b.items():
        scale = ref.abs().max().item()
        assert torch.allclose(a[k], ref, rtol=1e-5, atol=1e-6 * max(scale, 1e-30)), k


def test_binning_path_at_the_bit_budget_edges(native_lib):
    """Pure host query (no GPU): per tile above the one-sweep size (512 k), while the tile id has <= 16 bits and the index
    fits beside the low depth bits, P <= 2^(37 - tile bits); the radix_scanned option forces either path at any size."""
    lib = native_lib
    assert lib.mgs_binning_path(2_000_000, 1920, 1080) == 1            # C5: 8160 tiles, 13 bits
    assert lib.mgs_binning_path(512 * 1024, 1920, 1080) == 0           # one-sweep size: the global chain
    assert lib.mgs_binning_path(512 * 1024 + 1, 1920, 1080) == 1
    assert lib.mgs_binning_path(1 << 24, 1920, 1080) == 1              # 2^(37 - 13)
    assert lib.mgs_binning_path((1 << 24) + 1, 1920, 1080) == 0
    assert lib.mgs_binning_path(1 << 22, 3840, 2160) == 1              # 32 400 tiles, 15 bits: 2^22
    assert lib.mgs_binning_path((1 << 22) + 1, 3840, 2160) == 0
    assert lib.mgs_binning_path(1 << 21, 4096, 4096) == 1              # 65 536 tiles: 16 bits, 2^21
    assert lib.mgs_binning_path((1 << 21) + 1, 4096, 4096) == 0
    assert lib.mgs_binning_path(600_000, 4112, 4096) == 0              # 17 tile bits: a third tile-sort pass
    assert lib.mgs_binning_path(600_000, 64, 64) == 1                  # 16 tiles: no low depth bits in the value
    assert lib.mgs_binning_path(0, 640, 480) == 0
    with options(radix_scanned=1):
        assert lib.mgs_binning_path(5000, 640, 480) == 1
        assert lib.mgs_binning_path((1 << 26) - 1, 640, 480) == 1     # 1200 tiles: 11 bits, any P the library takes
    with options(radix_scanned=0):
        assert lib.mgs_binning_path(2_000_000, 1920, 1080) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("P,intr,seed", [(5000, "fr3_office", 0), (20000, "replica", 7)])
def test_per_tile_order_matches_the_global_sort_and_the_oracle(native_lib, P, intr, seed):
    from oracle import OracleSettings, rasterize
    sc = make_scene(P, intr, seed=seed)
    a, b = _tables(native_lib, sc, 1), _tables(native_lib, sc, 0)
    _same_tables(a, b)
    o = rasterize(sc.means3D, None, sc.opacities, scene_settings(sc, OracleSettings), colors_precomp=sc.colors,
                  scales=sc.scales.repeat(1, 3), rotations=sc.rotations)
    assert torch.equal(a["ranges"].cpu().long(), o.aux["ranges"])
    assert torch.equal(a["point_list"].cpu().long(), o.aux["point_list"])
    assert torch.equal(a["tiles_touched"].cpu().long(), o.aux["geom"]["tiles_touched"])
    _same_grads(native_lib, sc)


@pytest.mark.gpu
def test_exact_depth_ties_keep_index_order(native_lib):
    sc = make_scene(8000, "fr3_office", seed=3)
    f = lambda t: t.clone()  # noqa: E731
    means, scales, rots, opac, cols = f(sc.means3D), f(sc.scales), f(sc.rotations), f(sc.opacities), f(sc.colors)
    for t in (means, scales, rots, opac, cols):                     # every 7th Gaussian repeats the one before it
        t[7::7] = t[6:-1:7][: t[7::7].shape[0]]
    sc = sc._replace(means3D=means, scales=scales, rotations=rots, opacities=opac, colors=cols)
    a, b = _tables(native_lib, sc, 1), _tables(native_lib, sc, 0)
    dk = a["depth_key"].long()
    assert bool((dk[7::7] == dk[6:-1:7][: dk[7::7].shape[0]]).all())
    _same_tables(a, b)
    _same_grads(native_lib, sc)


@pytest.mark.gpu
def test_depths_beyond_the_narrow_range(native_lib):
    """Depths >= 13 107 units do not fit 27 bits: the pairs carry them clamped, and the kernel re-sorts each tile's
    trailing run of clamped keys by the full depth key."""
    K = 4000.0
    sc = make_scene(20000, "fr3_office", seed=11, near_fraction=0.0)
    sc = sc._replace(means3D=sc.means3D * K, scales=sc.scales * K, t=sc.t * K)
    a, b = _tables(native_lib, sc, 1), _tables(native_lib, sc, 0)
    vis = a["radii"] > 0
    depth = a["rec"][:, 11]
    assert float(depth[vis].max()) > 13107.2 > float(depth[vis].min())
    _same_tables(a, b)
    _same_grads(native_lib, sc)


@pytest.mark.gpu
def test_lists_longer_than_the_lds_take_the_global_segment_sort(native_lib):
    """Large splats: some tiles hold more than the kernel's 1024 LDS slots (sorted in global memory), the others not."""
    sc = make_scene(12000, "fr3_office", seed=4, mean_radius_px=80.0)
    a, b = _tables(native_lib, sc, 1), _tables(native_lib, sc, 0)
    n = (a["ranges"][:, 1] - a["ranges"][:, 0]).long()
    assert int((n > 1024).sum()) > 0 and int(((n > 0) & (n <= 1024)).sum()) > 0
    _same_tables(a, b)
    _same_grads(native_lib, sc)


@pytest.mark.gpu
def test_capacity_below_the_instance_count(native_lib):
    """Capacity mode with fewer slots than instances: both paths report the overflow and neither reads or writes past
    the capacity (the per-tile kernel clamps its ranges to the live count)."""
    from monogs_amd.debug import RawForward
    sc = make_scene(20000, "replica", seed=2)
    status = {}
    for value in (1, 0):
        with options(radix_scanned=value):
            f = RawForward(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc), zero=True)
            R = f.preprocess()
            f.render(R // 2, capacity=True)
            assert native_lib.mgs_binning_path(f.P, f.W, f.H) == value
            status[value] = (R, int(f.status.item()))
            assert bool(torch.isfinite(f.color).all())
    assert status[1] == status[0] and status[1][1] != 0
