"""Banded tile sort (option "tile_sort_banded" = 1, the default where it applies) against the two tile-sort passes (= 0): the
same tables bit for bit.

On the per-tile path, with a tile id wider than 8 bits and at most 32 bands of 256 tiles, preprocess counts every scan block's
instances per band, scan_blocks_kernel scans the counts along each band, emit_banded_kernel writes the pairs grouped by band
and ONE segmented 8-bit pass orders each band (csrc/binning.hip, csrc/radix_sort.hip).  "radix_scanned" = 1 forces the per-tile
path at small P, as in test_gpu_tile_depth_sort.py.  The shapes are the smallest at which it can go wrong: 336 x 272 (357
tiles, 2 bands) and 640 x 480 (1 200 tiles, 5 bands)."""
import pytest
import torch

from monogs_amd.debug import RawForward, options
from monogs_amd.synthetic import make_scene, scene_settings

DEV = "cuda:0"
SMALL = dict(fx=300.0, fy=300.0, cx=168.0, cy=136.0, W=336, H=272)          # 21 x 17 tiles: tile 255 | 256 is row 12, column 3 | 4
CANARY = 0x5A


def _settings(sc):
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    return scene_settings(sc, GaussianRasterizationSettings, device=DEV)


def _raw(sc):
    return RawForward(_settings(sc), sc.means3D.to(DEV), sc.opacities.to(DEV), colors_precomp=sc.colors.to(DEV),
                      scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV), zero=True)


def _with_splats(sc, splats, at=0):
    """`sc` with one isotropic Gaussian per (px, py, sigma_px, z) inserted at index `at`."""
    i = sc.intr
    pc = torch.tensor([[(px - i["cx"]) / i["fx"] * z, (py - i["cy"]) / i["fy"] * z, z] for px, py, _, z in splats])
    means = (pc - sc.t[None, :]) @ sc.R
    scales = torch.tensor([[s * z / i["fx"]] for _, _, s, z in splats])
    n = len(splats)
    ins = lambda old, new: torch.cat([old[:at], new.to(old.dtype), old[at:]]).contiguous()          # noqa: E731
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1)
    return sc._replace(means3D=ins(sc.means3D, means), scales=ins(sc.scales, scales), rotations=ins(sc.rotations, q),
                       opacities=ins(sc.opacities, torch.full((n, 1), 0.6)), colors=ins(sc.colors, torch.full((n, 3), 0.5)))


def _subset(sc, keep):
    keep = keep.cpu()
    return sc._replace(means3D=sc.means3D[keep].contiguous(), scales=sc.scales[keep].contiguous(),
                       rotations=sc.rotations[keep].contiguous(), opacities=sc.opacities[keep].contiguous(),
                       colors=sc.colors[keep].contiguous())


def _rects(sc):
    """Per Gaussian: first and last tile id of its rectangle, its width, height and tile count (0: culled), corner tile id."""
    with options(radix_scanned=1):
        f = _raw(sc)
        f.preprocess()
    r = f.table("geometry.rect").reshape(-1, 2).long()
    gx = (f.W + 15) // 16
    x0, y0, w, h = r[:, 0] & 0xFFFF, r[:, 0] >> 16, r[:, 1] & 0xFFFF, (r[:, 1] >> 16) & 0xFFFF
    first = y0 * gx + x0
    return dict(first=first, last=first + (h - 1).clamp_min(0) * gx + (w - 1).clamp_min(0), w=w, h=h, n=w * h, gx=gx)


def _render(f, R, capacity):
    """RawForward.render into a binning scratch filled with a canary and followed by a page of it (the render call allocates
    its scratch with torch.empty: for its duration that hands out the front of a larger, pre-filled buffer); returns what
    must still hold the canary afterwards: the page behind the scratch and the alignment padding behind each of the four pair
    buffers (a sub-buffer starts on a multiple of 256 bytes)."""
    made, real_empty = [], torch.empty

    def canary_empty(n, *args, **kw):
        big = torch.full((n + 4096,), CANARY, dtype=torch.uint8, device=kw.get("device", DEV))
        made.append(big)
        return big[:n]

    torch.empty = canary_empty
    try:
        f.render(R, capacity=capacity)
    finally:
        torch.empty = real_empty
    (big,) = made
    guard = [big[f.binning.numel():]]
    for name in ("binning.keys_a", "binning.keys_b", "binning.vals_a", "binning.vals_b"):
        t = f.table(name)
        end = t.data_ptr() + 4 * t.numel() - big.data_ptr()
        guard.append(big[end:end + (-(t.data_ptr() + 4 * t.numel())) % 256])
    return guard


def _run(sc, banded, mode):
    """One forward.  mode: "exact", "capacity" (room for 1.5 R + 1) or "overflow" (room for R / 2, made odd so that the pair
    buffers end inside a 256-byte line)."""
    with options(radix_scanned=1, tile_sort_banded=banded):
        f = _raw(sc)
        assert f.lib.mgs_binning_path(f.P, f.W, f.H) == 1
        R = f.preprocess()
        room = {"exact": R, "capacity": R + R // 2 + 1, "overflow": (R // 2) | 1}[mode]
        guard = _render(f, room, mode != "exact")
        bands = f.lib.mgs_debug_last_tile_sort_bands()
    out = dict(R=R, bands=bands, status=int(f.status.item()), color=f.color, depth=f.depth, opacity=f.opacity,
               n_touched=f.n_touched, ranges=f.table("image.ranges").clone(), guard_ok=all(bool((g == CANARY).all()) for g in guard))
    live = min(R, room)              # (with half the room both chains keep the first `room` slots of the Gaussian-major order)
    out.update(point_list=f.table("binning.point_list")[:live].clone(), keys=f.table("binning.keys_a")[:live].clone())
    if mode != "exact":
        out.update(count=f.table("binning.count")[:2].clone())
    return out


def _same(sc, bands):
    """Banded against the two passes, in exact mode, in capacity mode, and with half the room."""
    for mode in ("exact", "capacity", "overflow"):
        a, b = _run(sc, 1, mode), _run(sc, 0, mode)
        assert a["bands"] == bands and b["bands"] == 0, (mode, a["bands"], b["bands"])
        assert a["R"] == b["R"] > 0
        assert a["guard_ok"] and b["guard_ok"], mode
        assert a["status"] == b["status"], (mode, a["status"], b["status"])
        assert (a["status"] != 0) == (mode == "overflow"), (mode, a["status"])
        if mode != "exact":
            assert torch.equal(a["count"], b["count"]), (mode, a["count"], b["count"])
        for k in ("point_list", "keys", "ranges", "n_touched", "color", "depth", "opacity"):
            assert torch.equal(a[k], b[k]), (mode, k)


@pytest.mark.gpu
def test_two_bands_row_cut_at_the_band_boundary(native_lib):
    """336 x 272, P not a multiple of 256; a rectangle row holds the tile ids 255 | 256."""
    sc = _with_splats(make_scene(3001, SMALL, seed=1), [(64.0, 200.0, 5.0, 2.0)], at=1500)
    r = _rects(sc)
    rows = torch.arange(int(r["h"].max()), device=DEV)[None, :]
    lo = r["first"][:, None] + rows * r["gx"]                                 # first tile id of every row of every rectangle
    cut = (rows < r["h"][:, None]) & (r["n"][:, None] > 0) & ((lo >> 8) != ((lo + r["w"][:, None] - 1) >> 8))
    assert bool(cut[1500].any()) and int(cut.any(dim=1).sum()) >= 2
    _same(sc, 2)


@pytest.mark.gpu
def test_five_bands_rectangle_over_three_bands(native_lib):
    sc = _with_splats(make_scene(20000, "fr3_office", seed=7), [(320.0, 240.0, 40.0, 3.0)], at=7)
    r = _rects(sc)
    assert int(((r["last"] >> 8) - (r["first"] >> 8))[r["n"] > 0].max()) >= 2
    _same(sc, 5)


@pytest.mark.gpu
def test_empty_band_in_the_middle_and_all_instances_in_one_band(native_lib):
    sc = make_scene(6000, "fr3_office", seed=3)
    r = _rects(sc)
    vis = r["n"] > 0
    outside = vis & ((r["last"] < 512) | (r["first"] >= 768))                 # nothing in band 2 (tiles 512..767)
    hollow = _subset(sc, outside | ~vis)
    rh = _rects(hollow)
    v = rh["n"] > 0
    assert int((v & (rh["last"] < 512)).sum()) > 0 and int((v & (rh["first"] >= 768)).sum()) > 0
    _same(hollow, 5)
    inside = vis & ((r["first"] >> 8) == 1) & ((r["last"] >> 8) == 1)        # everything in band 1
    assert int(inside.sum()) > 300
    _same(_subset(sc, inside), 5)


@pytest.mark.gpu
def test_scan_block_without_instances_and_block_of_big_splats(native_lib):
    """A 256-Gaussian scan block that emits nothing (the near-culled Gaussians come first), and blocks whose instances
    exceed the emission kernel's 1024-slot stage many times over."""
    sc = make_scene(5000, "fr3_office", seed=5, near_fraction=0.06)
    assert int(_rects(sc)["n"][:256].sum()) == 0
    _same(sc, 5)
    big = make_scene(2500, "fr3_office", seed=4, mean_radius_px=80.0)
    n = _rects(big)["n"]
    assert int(n[:2304].reshape(9, 256).sum(dim=1).max()) > 4 * 1024
    _same(big, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,why", [(256, 256, "256 tiles: one digit"), (2048, 1040, "8 320 tiles: 33 bands")])
def test_other_images_keep_the_two_pass_chain(native_lib, W, H, why):
    intr = dict(fx=0.8 * W, fy=0.8 * W, cx=W / 2, cy=H / 2, W=W, H=H)
    sc = make_scene(3000, intr, seed=2)
    a, b = _run(sc, 1, "exact"), _run(sc, 0, "exact")
    assert a["bands"] == 0 and b["bands"] == 0, why
    for k in ("point_list", "ranges", "n_touched", "color"):
        assert torch.equal(a[k], b[k]), k


def test_tile_sort_banded_option_and_getter_are_known(native_lib):
    """Pure host query (no GPU)."""
    for v in (0, 1, -1):
        assert native_lib.mgs_debug_set_option(b"tile_sort_banded", v) == 0
    assert native_lib.mgs_debug_last_tile_sort_bands() >= 0
