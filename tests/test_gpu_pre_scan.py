"""Per-tile path: the scan of tiles touched folded into the per-Gaussian forward kernel (option "pre_scan" = 1, the default:
256-Gaussian scan blocks written by preprocess, one launch over the block sums) against the scan as launches of its own
(= 0, 2048-Gaussian blocks): the same tables and images bit for bit, and the oracle's tables where it is affordable.
Scenes are forced onto the per-tile path (radix_scanned = 1) at 640x480.  Sizes: a single Gaussian, a partial block, exactly
one block, one past the block boundary, a partial third block, and two sizes with many blocks (20 000: 79 blocks of 256,
10 of 2048).  Both emission orders of duplicate_kernel (Gaussian-major, slot-major) decode their slots with the
reciprocal multiply of dup_divmod (tests/test_dup_slot_decode.py) from the 16-byte LDS entries."""
import functools

import pytest
import torch

from monogs_amd.synthetic import make_scene, scene_settings
from oracle import OracleSettings, rasterize

DEV = "cuda:0"
KEYS = ("tiles_touched", "ranges", "point_list", "tile_sorted", "radii", "n_touched", "n_contrib", "color", "depth",
        "opacity")


def _settings(sc):
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    return scene_settings(sc, GaussianRasterizationSettings, device=DEV)


def _args(sc):
    return dict(colors_precomp=sc.colors.to(DEV), scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV))


def _tables(lib, sc, **kw):
    from monogs_amd.debug import forward_tables, options
    with options(radix_scanned=1, **kw):                    # (the per-tile path, whatever the size)
        t = forward_tables(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc))
    assert t["depth_path"] == "per_tile" and t["status"] == 0
    return t


def _same(a, b):
    assert a["num_rendered"] == b["num_rendered"]
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def _oracle(P):
    sc = make_scene(P, "fr3_office", seed=P % 13)
    o = rasterize(sc.means3D, None, sc.opacities, scene_settings(sc, OracleSettings), colors_precomp=sc.colors,
                  scales=sc.scales.repeat(1, 3), rotations=sc.rotations)
    return o


def test_pre_scan_option_is_known(native_lib):
    """Host-only: the option exists, takes 0 / 1, and -1 restores the default."""
    for v in (0, 1, -1):
        assert native_lib.mgs_debug_set_option(b"pre_scan", v) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 255, 256, 257, 513, 5000, 20000])
def test_pre_scan_matches_the_scan_launches(native_lib, P):
    sc = make_scene(P, "fr3_office", seed=P % 13)
    a, b = _tables(native_lib, sc, pre_scan=1), _tables(native_lib, sc, pre_scan=0)
    _same(a, b)
    if P >= 5000:               # and the oracle's tables, as test_gpu_parity.py::test_forward_tables_bit_exact
        o = _oracle(P)
        assert a["num_rendered"] == o.aux["num_rendered"]
        assert torch.equal(a["radii"].cpu(), o.radii)
        assert torch.equal(a["tiles_touched"].cpu().long(), o.aux["geom"]["tiles_touched"])
        assert torch.equal(a["ranges"].cpu().long(), o.aux["ranges"])
        assert torch.equal(a["point_list"].cpu().long(), o.aux["point_list"])
        keys = torch.from_numpy(o.aux["keys"].astype("int64"))          # tile << 32 | depth bits, sorted
        assert torch.equal(a["tile_sorted"].cpu().long(), keys >> 32)


@pytest.mark.gpu
def test_pre_scan_both_emission_orders_on_large_splats(native_lib):
    """Rectangles of hundreds of tiles: slot-major emission (the 64-way search adds the block sums at the scan's
    granularity) and Gaussian-major emission, each under both scans; all four the same tables."""
    sc = make_scene(12000, "fr3_office", seed=4, mean_radius_px=80.0)
    ref = _tables(native_lib, sc, pre_scan=0, dup_slot_major=0)
    assert ref["num_rendered"] > 6 * 12000
    assert int(ref["tiles_touched"].max()) > 64             # rectangles spanning more than one 64-slot chunk
    for pre, major in ((1, 0), (1, 1), (0, 1)):
        _same(_tables(native_lib, sc, pre_scan=pre, dup_slot_major=major), ref)


@pytest.mark.gpu
def test_pre_scan_capacity_below_the_instance_count(native_lib):
    """Capacity mode with half the slots (the shape of test_gpu_tile_sort_fused.py's case): the same overflow word, images,
    ranges and live point list under both scans."""
    from monogs_amd.debug import RawForward, options
    sc = make_scene(20000, "replica", seed=2)
    out = {}
    for pre in (1, 0):
        with options(radix_scanned=1, pre_scan=pre):
            f = RawForward(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), **_args(sc), zero=True)
            R = f.preprocess()
            f.render(R // 2, capacity=True)
            assert native_lib.mgs_binning_path(f.P, f.W, f.H) == 1
            ranges = f.table("image.ranges").reshape(-1, 2).clone()
            live = int(ranges[:, 1].max())
            out[pre] = dict(over=int(f.status.item()), R=R, color=f.color.clone(), depth=f.depth.clone(),
                            opacity=f.opacity.clone(), n_touched=f.n_touched.clone(), radii=f.radii.clone(), ranges=ranges,
                            live=live, point_list=f.table("binning.point_list")[:live].clone())
    a, b = out[1], out[0]
    assert a["over"] != 0 and a["over"] == b["over"] and a["R"] == b["R"]
    assert 0 < a["live"] <= a["R"] // 2
    for k in ("color", "depth", "opacity", "n_touched", "radii", "ranges", "point_list"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [1, 0])
def test_pre_scan_every_gaussian_behind_the_camera(native_lib, pre):
    """No instance at all (R = 0): every block total is 0, every range {0, 0}, the image is the background."""
    sc = make_scene(3000, "fr3_office", seed=1, bg=(0.2, 0.4, 0.6))
    pv = sc.means3D @ sc.R.T + sc.t                         # view space: mirror every mean to behind the camera
    pv[:, 2] = -pv[:, 2]
    sc = sc._replace(means3D=((pv - sc.t) @ sc.R).contiguous())
    t = _tables(native_lib, sc, pre_scan=pre)
    assert t["num_rendered"] == 0
    assert int(t["radii"].abs().max()) == 0 and int(t["n_touched"].abs().max()) == 0
    assert int(t["tiles_touched"].abs().max()) == 0
    assert int(t["ranges"].abs().max()) == 0
    assert int(t["n_contrib"].abs().max()) == 0
    bg = sc.bg.to(DEV).reshape(3, 1, 1)
    assert torch.equal(t["color"], bg.expand_as(t["color"]).contiguous())
    assert float(t["opacity"].abs().max()) == 0.0 and float(t["depth"].abs().max()) == 0.0
