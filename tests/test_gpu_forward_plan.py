"""Every route of the forward plan (csrc/forward_plan.h) renders the same images and the same tile lists, and the emission that
is launched is the one the plan names: 640 x 480, 5000 random Gaussians of small extent, under the option sets that pick the
routes ("radix_scanned" = 1 forces the per-tile path at this size, as in test_gpu_tile_depth_sort.py).  The plan is asked
through ``mgs_debug_forward_plan``; what it must answer is tests/test_forward_plan_host.py's subject."""
import ctypes as C

import pytest
import torch

from monogs_amd import _lib
from monogs_amd.debug import RawForward, options
from monogs_amd.synthetic import make_scene, scene_settings

DEV = "cuda:0"
OPTION_SETS = [{}, dict(radix_scanned=1), dict(radix_scanned=1, pre_scan=0), dict(radix_scanned=1, tile_sort_banded=0),
               dict(radix_scanned=1, dup_slot_major=1), dict(radix_scanned=1, tile_sort_fused=0), dict(scan_small=0)]
# (the word indices of include/monogs_raster.h, MGS_PLAN_*)
PLAN_PER_TILE, PLAN_SCAN_ITEMS, PLAN_SCAN_SMALL, PLAN_SLOT_MAJOR, PLAN_BANDS, PLAN_TILE_SORT_FUSED, PLAN_WORDS = 10, 11, 14, 20, 21, 26, 30


def _forward(sc, opt, capacity_factor=0):
    """One whole forward under `opt`: the outputs, the live tile lists, the bands of the emission launched and the plan's words
    for what was rendered (exact: the R the forward reported; capacity mode: room for capacity_factor * R)."""
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    with options(**opt):
        f = RawForward(scene_settings(sc, GaussianRasterizationSettings, device=DEV), sc.means3D.to(DEV), sc.opacities.to(DEV),
                       colors_precomp=sc.colors.to(DEV), scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV), zero=True)
        R = f.preprocess()
        room = capacity_factor * R if capacity_factor else R
        f.render(room, capacity=capacity_factor != 0)
        launched = f.lib.mgs_debug_last_tile_sort_bands()
        plan = (C.c_uint64 * PLAN_WORDS)()
        _lib.check(f.lib.mgs_debug_forward_plan(f.P, f.W, f.H, int(f.cam.flags), room, 1 if capacity_factor else 0, plan),
                   "mgs_debug_forward_plan")
    return dict(R=R, launched=launched, plan=[int(w) for w in plan], status=int(f.status.item()), color=f.color.clone(),
                depth=f.depth.clone(), opacity=f.opacity.clone(), ranges=f.table("image.ranges").clone(),
                point_list=f.table("binning.point_list")[:R].clone())


@pytest.fixture(scope="module")
def renders():
    sc = make_scene(5000, "fr3_office", seed=11, mean_radius_px=4.0)
    return sc, [_forward(sc, opt) for opt in OPTION_SETS]


@pytest.mark.gpu
def test_the_emission_launched_is_the_plans_and_every_route_gives_the_same_tables(native_lib, renders):
    _, runs = renders
    ref = runs[0]
    assert ref["R"] > 5000 and ref["status"] == 0
    for opt, r in zip(OPTION_SETS, runs):
        assert r["launched"] == r["plan"][PLAN_BANDS], (opt, r["launched"], r["plan"][PLAN_BANDS])
        assert r["R"] == ref["R"] and r["status"] == 0, opt
        for k in ("color", "depth", "opacity", "ranges", "point_list"):
            assert torch.equal(r[k], ref[k]), (opt, k)
    # the seven sets do take seven routes: (per_tile, scan_items, scan_small, slot_major, bands, tile_sort_fused) of each
    route = lambda r: tuple(r["plan"][i] for i in (PLAN_PER_TILE, PLAN_SCAN_ITEMS, PLAN_SCAN_SMALL, PLAN_SLOT_MAJOR, PLAN_BANDS, PLAN_TILE_SORT_FUSED))  # noqa: E731
    assert [route(r) for r in runs] == [(0, 2048, 1, 0, 0, 0), (1, 256, 0, 0, 5, 1), (1, 2048, 1, 0, 0, 1), (1, 256, 0, 0, 0, 1),
                                        (1, 256, 0, 1, 0, 1), (1, 256, 0, 0, 5, 0), (0, 2048, 0, 0, 0, 0)]


@pytest.mark.gpu
def test_capacity_mode_at_twice_the_count_follows_the_plan_for_that_capacity(native_lib, renders):
    sc, runs = renders
    ref = runs[0]
    cap = _forward(sc, dict(radix_scanned=1), capacity_factor=2)
    assert cap["R"] == ref["R"] and cap["status"] == 0
    assert cap["launched"] == cap["plan"][PLAN_BANDS] == 5
    for k in ("color", "depth", "opacity", "ranges", "point_list"):
        assert torch.equal(cap[k], ref[k]), k
