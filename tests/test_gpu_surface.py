"""Median depth, depth variance and depth normals on the device (csrc/surface.hip, monogs_amd/surface.py) against the CPU mirror of
the specification (tests/surface_mirror.py, which tests/test_surface_host.py ties to the oracle), against the rasteriser's own
output, and through ``fuse_map`` / ``eval_geometry`` (run on the MI355X box: pytest -m gpu).

Bars.  On the pixels the oracle does not flag ambiguous (a decision within a few ulps of its threshold; their share < 1e-3, the cap
of tests/test_gpu_parity.py): the median contributor is the mirror's, its depth is the oracle's float32 depth of that Gaussian bit for
bit, the pixels without a median are the mirror's.  The variance and the normals follow the rule DESIGN.md uses for the pose tangents:
max |hip - m64| <= 4 x max |m32 - m64|, m64 / m32 the mirror with float64 / float32 arithmetic, the right-hand side recomputed here.

All scenes render at 104 x 72 (7 x 5 tiles, a half tile on both far edges); tests/surface_mirror.py lists them and
tests/test_surface_host.py what each must keep exercising.
"""
import functools
import math

import numpy as np
import pytest
import torch

import surface_mirror as M
import tsdf_cases as TC
from monogs_amd.debug import options
from monogs_amd.synthetic import scene_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = M.INTR["H"], M.INTR["W"]
WALK_SCENES = ["multi", "veil", "haze", "long", "sparse", "stack"]


class _Intr:                      # what depth_normals reads of an intrinsics object
    def __init__(self, d):
        self.fx, self.fy, self.cx, self.cy = d["fx"], d["fy"], d["cx"], d["cy"]


INTR = _Intr(M.INTR)


@functools.lru_cache(maxsize=None)
def _mirror(name, sum_dtype=torch.float64, min_opacity=0.0, max_std=0.0):
    """Computed once per argument set, never modified."""
    return M.surface_mirror(M.oracle(name).aux, H, W, sum_dtype=sum_dtype, min_opacity=min_opacity, max_std=max_std)


@functools.lru_cache(maxsize=None)
def _variance_bound(name):
    """4 x max |m32 - m64| over the clear pixels: what float32 sums in blend order cost on this scene."""
    clear = ~M.oracle(name).aux["ambiguous"]
    m64, m32 = _mirror(name).depth_var, _mirror(name, torch.float32).depth_var
    return 4.0 * (m32.double() - m64)[clear].abs().max().item()


def _forward(sc, grad=True):
    """A rasteriser forward of the scene; returns (color, radii, depth, opacity, leaves)."""
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(grad)  # noqa: E731
    leaves = dict(means3D=leaf(sc.means3D), opacities=leaf(sc.opacities), colors_precomp=leaf(sc.colors), scales=leaf(M.scales3(sc)),
                  rotations=leaf(sc.rotations))
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=grad)
    leaves["theta"] = torch.zeros(3, device=DEV, requires_grad=grad)
    leaves["rho"] = torch.zeros(3, device=DEV, requires_grad=grad)
    color, radii, depth, opacity, n_touched = GaussianRasterizer(st)(**leaves)
    return color, radii, depth, opacity, leaves


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the median against the mirror -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WALK_SCENES)
def test_median_vs_mirror(native_lib, name):
    from monogs_amd import surface_depth
    o, m = M.oracle(name), _mirror(name)
    clear = ~o.aux["ambiguous"]
    color, *_ = _forward(M.scene(name))
    sd = surface_depth(color, want_id=True)
    assert sd.median.shape == sd.median_id.shape == sd.variance.shape == (H, W)
    assert sd.median.dtype == sd.variance.dtype == torch.float32 and sd.median_id.dtype == torch.int32
    ids, med = sd.median_id.cpu().long(), sd.median.cpu()
    print(f"{name}: ambiguous {int((~clear).sum())}, median ids that differ on clear pixels {int((ids != m.median_id)[clear].sum())}, "
          f"without a median {int((ids < 0).sum())} (mirror {int((m.median_id < 0).sum())})")
    assert (~clear).float().mean().item() < 1e-3
    assert torch.equal(ids[clear], m.median_id[clear])
    assert torch.equal((ids < 0)[clear], (m.median_pos == 0)[clear])
    z = o.aux["geom"]["depth"]
    assert z.dtype == torch.float32
    expect = torch.where(ids >= 0, z[ids.clamp_min(0)], torch.zeros(()))
    assert torch.equal(med.view(torch.int32)[clear], expect.view(torch.int32)[clear])       # the record's float, bit for bit
    if name == "stack":
        x0, y0 = (int(round(float(v))) for v in o.aux["geom"]["xy"][0])
        assert (ids[y0 - 1:y0 + 2, x0 - 1:x0 + 2] == 1).all() and (med[y0 - 1:y0 + 2, x0 - 1:x0 + 2] == z[1]).all()


# ---- 2. the variance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WALK_SCENES)
def test_variance_vs_mirror(native_lib, name):
    from monogs_amd import surface_depth
    clear = ~M.oracle(name).aux["ambiguous"]
    m64 = _mirror(name).depth_var
    bound = _variance_bound(name)
    color, *_ = _forward(M.scene(name))
    var = surface_depth(color, want=("variance",)).variance.cpu()
    err = (var.double() - m64)[clear].abs().max().item()
    print(f"{name}: max |hip - m64| = {err:.3e}, 4 x max |m32 - m64| = {bound:.3e}, ratio to the bound {err / max(bound, 1e-300):.2f}, "
          f"largest variance {m64.max().item():.3e}")
    assert (var >= 0).all()
    assert (var[_mirror(name).O == 0] == 0).all()                  # no contributor: exactly 0
    assert err <= bound


# ---- 3. the gates -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["veil", "multi"])
@pytest.mark.parametrize("min_opacity,max_std", [(0.9, 0.0), (0.0, 0.05), (0.9, 0.05), (0.6, 1.0)])
def test_gates_vs_mirror(native_lib, name, min_opacity, max_std):
    from monogs_amd import surface_depth
    o = M.oracle(name)
    m = _mirror(name, torch.float64, min_opacity, max_std)
    free = _mirror(name)
    exempt = o.aux["ambiguous"].clone()
    if min_opacity > 0:
        exempt |= ((1.0 - o.aux["final_T"][0]).double() - min_opacity).abs() <= 1e-6
    if max_std > 0:
        max_var = float(torch.tensor(max_std, dtype=torch.float32) ** 2)
        exempt |= (free.depth_var - max_var).abs() <= _variance_bound(name)
    color, *_ = _forward(M.scene(name))
    sd = surface_depth(color, want=("median", "variance") if max_std > 0 else ("median",), min_opacity=min_opacity, max_std=max_std,
                       want_id=True)
    ids, med = sd.median_id.cpu().long(), sd.median.cpu()
    cleared, cleared_m = (ids < 0) & (free.median_id >= 0), m.gated & (free.median_id >= 0)
    print(f"{name} min_opacity {min_opacity} max_std {max_std}: cleared {int(cleared.sum())} (mirror {int(cleared_m.sum())}), "
          f"exempt {int(exempt.sum())}, kept {int((ids >= 0).sum())}")
    assert exempt.float().mean().item() < 1e-3
    assert torch.equal(cleared[~exempt], cleared_m[~exempt])
    assert int(cleared_m.sum()) > 0                                         # the gate bites ...
    if (min_opacity, max_std) == (0.6, 1.0):
        assert int((ids >= 0).sum()) > 500                                  # ... and, at this pair, not everywhere (on veil the others clear all)
    assert torch.equal(ids[~exempt], m.median_id[~exempt]) and torch.equal(med[~exempt], m.median_depth[~exempt])
    assert torch.equal(med != 0, ids >= 0)
    if max_std > 0:                                                         # the gates leave the variance plane alone
        assert torch.equal(sd.variance, surface_depth(color, want=("variance",)).variance)


# ---- 4. against the rasteriser's own output ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WALK_SCENES)
def test_median_vs_the_forward_opacity(native_lib, name):
    from monogs_amd import surface_depth
    color, _, _, opacity, _ = _forward(M.scene(name))
    sd = surface_depth(color, want=("median",), want_id=True)
    op = opacity.detach()[0]
    away = (op - 0.5).abs() > 1e-5
    assert torch.equal((sd.median_id >= 0)[away], (op >= 0.5)[away])
    assert torch.equal(sd.median != 0, sd.median_id >= 0)
    assert int(sd.median_id.max()) < M.scene(name).means3D.shape[0]


# ---- 5. the early leave changes nothing; two calls agree -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", WALK_SCENES)
def test_early_leave_and_reproducibility(native_lib, name):
    from monogs_amd import surface_depth
    color, *_ = _forward(M.scene(name))
    both = surface_depth(color, want_id=True)
    alone = surface_depth(color, want=("median",), want_id=True)
    assert alone.variance is None and surface_depth(color, want=("variance",)).median is None
    assert torch.equal(alone.median.view(torch.int32), both.median.view(torch.int32)) and torch.equal(alone.median_id, both.median_id)
    assert _same(surface_depth(color, want_id=True), both) and _same(surface_depth(color, want=("median",), want_id=True), alone)
    assert torch.equal(surface_depth(color, want=("median",)).median, alone.median)          # median_id is optional


# ---- 6. both binning paths, both forward modes ------------------------------------------------------------------------------------
def test_binning_paths_and_forward_modes(native_lib):
    from monogs_amd import rasterizer as R, surface_depth
    sc = M.scene("long")
    P = sc.means3D.shape[0]
    run = lambda color: surface_depth(color, want_id=True)  # noqa: E731
    R.set_sync_free(False)
    assert native_lib.mgs_binning_path(P, W, H) == 0
    ref = run(_forward(sc)[0])                            # exact mode, global depth sort (records the capacity hint)
    with options(radix_scanned=1):
        assert native_lib.mgs_binning_path(P, W, H) == 1
        per_tile = run(_forward(sc)[0])
        try:
            R.set_sync_free(True, headroom=1.2)
            color = _forward(sc)[0]
            assert color.grad_fn.overflow is not None
            per_tile_cap = run(color)
            assert not R.check_overflow()
        finally:
            R.set_sync_free(False)
    try:
        R.set_sync_free(True, headroom=1.2)
        color = _forward(sc)[0]
        assert color.grad_fn.overflow is not None         # the capacity path ran
        cap = run(color)
        assert not R.check_overflow()
    finally:
        R.set_sync_free(False)
        R.forget_capacity(P, W, H)
    assert _same(per_tile, ref) and _same(cap, ref) and _same(per_tile_cap, ref)
    assert int((ref.median_id >= 0).sum()) == H * W


# ---- 7. beside the rasteriser's backward --------------------------------------------------------------------------------------------
def test_beside_the_rasteriser_backward(native_lib):
    """The call only reads: the scratch of the forward is the same bytes after it, the planes are the same before and after the
    rasteriser's backward, and the forward's outputs are bit-equal with and without the call in between.  The backward's gradients
    cannot be held to bit-equality: the blend backward adds its partial sums with float atomics, so two backward runs of ONE forward
    already differ in the last bits (the test prints how many elements of two plain runs differ).  What is exact is asserted exactly
    -- every byte the backward reads -- and the gradients to a relative L2 of 1e-6, ten float32 roundings."""
    from monogs_amd import surface_depth
    from monogs_amd.rasterizer import forward_scratch
    sc = M.scene("veil")
    gc, gd = sc.grad_color.to(DEV), sc.grad_depth.to(DEV)

    def run(between):
        color, radii, depth, opacity, leaves = _forward(sc)
        before = after = None
        if between:
            t = forward_scratch(color)                    # one request before the backward keeps the scratch
            arena, binning = t.arena.clone(), t.binning.clone()
            before = surface_depth(color, want_id=True)
            assert torch.equal(arena, t.arena) and torch.equal(binning, t.binning)
        ((color * gc).sum() + (depth * gd).sum()).backward()
        if between:
            after = surface_depth(color, want_id=True)
        outs = [color.detach().clone(), depth.detach().clone(), opacity.detach().clone()]
        return outs, {k: v.grad.clone() for k, v in leaves.items() if v.grad is not None}, before, after

    outs0, grads0, _, _ = run(False)
    _, grads_again, _, _ = run(False)
    outs1, grads1, before, after = run(True)
    assert _same(before, after) and int((before.median_id >= 0).sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(outs0, outs1))
    assert set(grads0) == set(grads1) and len(grads0) >= 7
    for k in grads0:
        rel = ((grads0[k] - grads1[k]).norm() / grads0[k].norm().clamp_min(1e-30)).item()
        print(f"{k}: {int((grads0[k] != grads_again[k]).sum())} elements differ between two plain runs, "
              f"{int((grads0[k] != grads1[k]).sum())} with the call in between (relative L2 {rel:.1e})")
        assert rel <= 1e-6, k
    # without the request the backward frees the scratch, and the call says so
    color, _, depth, _, _ = _forward(sc)
    ((color * gc).sum() + (depth * gd).sum()).backward()
    with pytest.raises(RuntimeError, match="surface_depth: the rasteriser's backward has already freed this forward's scratch"):
        surface_depth(color)


# ---- 8. a captured graph replays to the eager result ------------------------------------------------------------------------------------
def test_graph_replay(native_lib):
    from monogs_amd import depth_normals, rasterizer as R, surface_depth
    sc = M.scene("veil")
    P = sc.means3D.shape[0]

    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)          # every copy to the device happens before the capture
    args = dict(means3D=sc.means3D.to(DEV), opacities=sc.opacities.to(DEV), scales=M.scales3(sc).to(DEV), rotations=sc.rotations.to(DEV))
    args["means2D"] = torch.zeros_like(args["means3D"])
    colors = sc.colors.to(DEV).requires_grad_(True)                             # (a forward that keeps its tables)

    def work():
        color = GaussianRasterizer(st)(colors_precomp=colors, **args)[0]
        sd = surface_depth(color, min_opacity=0.3, max_std=2.0, want_id=True)
        return [sd.median, sd.median_id, sd.variance, depth_normals(sd.median, INTR, max_jump=0.5)]

    R.check_overflow()
    R.set_sync_free(False)
    eager = [t.clone() for t in work()]                   # exact: records the capacity hint of this map size
    handle, graph = R.graph_flags(), torch.cuda.CUDAGraph()
    try:
        with handle, torch.cuda.graph(graph):
            out = work()
        for _ in range(2):
            for t in out:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, eager):
                assert torch.equal(a, b)
        assert not R.check_overflow()
    finally:
        handle.release()
        R.clear_graph_flags()
        R.forget_capacity(P, W, H)
    assert int((eager[1] >= 0).sum()) > 0 and bool((eager[3] != 0).any())


# ---- 9. no Gaussians ------------------------------------------------------------------------------------------------------------------
def test_empty_map(native_lib):
    from monogs_amd import surface_depth
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    st = scene_settings(M.scene("sparse"), GaussianRasterizationSettings, device=DEV)
    e = lambda *s: torch.empty(*s, device=DEV)  # noqa: E731
    color = GaussianRasterizer(st)(means3D=e(0, 3), means2D=e(0, 3), opacities=e(0, 1), colors_precomp=e(0, 3).requires_grad_(True),
                                   scales=e(0, 3), rotations=e(0, 4))[0]
    sd = surface_depth(color, want_id=True)
    assert (sd.median == 0).all() and (sd.median_id == -1).all() and (sd.variance == 0).all()
    sd = surface_depth(color, want=("median",))
    assert (sd.median == 0).all() and sd.median_id is None and sd.variance is None


# ---- 10. depth normals -----------------------------------------------------------------------------------------------------------------
def _plane_depth(n, c):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return c / (n[0] * (xs + 0.5 - M.INTR["cx"]) / M.INTR["fx"] + n[1] * (ys + 0.5 - M.INTR["cy"]) / M.INTR["fy"] + n[2])


def _normals_case(name):
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    d = _plane_depth(n, -2.0).astype(np.float32)
    if name == "plane":
        return d, 0.0, n
    if name == "holes":
        d[20, 30], d[40, 50], d[5:9, 90:99] = 0.0, -1.0, 0.0
        return d, 0.0, n
    if name == "step":
        d[:, 60:] += 0.5
        return d, 0.2, n
    raise KeyError(name)


def _check_normals(got, depth32, max_jump, what):
    a = (M.INTR["fx"], M.INTR["fy"], M.INTR["cx"], M.INTR["cy"])
    m64 = M.depth_normals(depth32, *a, max_jump=max_jump, dtype=np.float64)
    m32 = M.depth_normals(depth32, *a, max_jump=max_jump, dtype=np.float32)
    bound = 4.0 * np.abs(m32.astype(np.float64) - m64).max()
    err = np.abs(got.astype(np.float64) - m64).max()
    print(f"{what}: max |hip - m64| = {err:.3e}, 4 x max |m32 - m64| = {bound:.3e}; elements that differ from m32: "
          f"{int((got != m32).sum())} of {got.size}; zero pixels {int((got == 0).all(0).sum())} (m64 {int((m64 == 0).all(0).sum())})")
    assert err <= bound
    return m64


@pytest.mark.parametrize("name", ["plane", "holes", "step"])
def test_depth_normals_vs_mirror(native_lib, name):
    from monogs_amd import depth_normals
    d, max_jump, n = _normals_case(name)
    got = depth_normals(torch.from_numpy(d).to(DEV), INTR, max_jump=max_jump)
    assert got.shape == (3, H, W) and got.dtype == torch.float32
    got = got.cpu().numpy()
    m64 = _check_normals(got, d, max_jump, name)
    zero = (got == 0).all(0)
    assert (zero == (m64 == 0).all(0)).all()                       # the border, the holes and the step: the mirror's zeros
    assert zero[0].all() and zero[-1].all() and zero[:, 0].all() and zero[:, -1].all()
    assert np.abs(got[:, ~zero] - n[:, None]).max() < 1e-3 if name != "step" else zero[1:-1, 59:61].all()
    assert np.abs(np.linalg.norm(got[:, ~zero], axis=0) - 1.0).max() < 1e-6
    if name == "plane":
        assert not zero[1:-1, 1:-1].any()
        assert torch.equal(depth_normals(torch.from_numpy(d).to(DEV)[None], INTR), torch.from_numpy(got).to(DEV))     # [1,H,W] too


@pytest.mark.parametrize("max_jump", [0.0, 0.05])
def test_depth_normals_of_the_median_depth(native_lib, max_jump):
    from monogs_amd import depth_normals, surface_depth
    color, *_ = _forward(M.scene("multi"))
    med = surface_depth(color, want=("median",)).median
    got = depth_normals(med, INTR, max_jump=max_jump).cpu().numpy()
    _check_normals(got, med.cpu().numpy(), max_jump, f"median depth of multi, max_jump {max_jump}")
    zero = (got == 0).all(0)
    assert 0 < int((~zero).sum()) and (max_jump == 0.0 or int(zero.sum()) > 2 * (H + W))
    # facing the camera: n . P <= 0 wherever there is a normal
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(xs + 0.5 - M.INTR["cx"]) / M.INTR["fx"], (ys + 0.5 - M.INTR["cy"]) / M.INTR["fy"], np.ones((H, W))])
    assert ((got * ray).sum(0)[~zero] <= 1e-6).all()


# ---- 11. fuse_map and eval_geometry on the room ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room_map():
    from monogs_amd.gaussian_map import GaussianMap
    frs, intr = TC.room_frames(DEV)
    for f in frs:
        f.update_RT(f.R_gt.clone(), f.T_gt.clone())
    gmap = GaussianMap(DEV)
    for f in frs[:3]:
        gmap.extend_from_frame(f, intr, downsample=4, init=True, point_size=1.0)
    gmap._opacity.data.fill_(4.0)                                # opaque splats (0.98): the render's opacity passes opacity_min unmapped
    return gmap, frs, intr


def test_fuse_map_mean_is_untouched_and_median_fuses(native_lib, room_map):
    from monogs_amd.sequences import room_surface_distance
    from monogs_amd.tsdf import TSDFVolume, fuse_map
    gmap, frs, intr = room_map
    bg = torch.zeros(3, device=DEV)
    views = frs[:3]
    make = lambda: TSDFVolume.for_bounds(TC.ROOM_LO, TC.ROOM_HI, 0.08, DEV)  # noqa: E731
    a, b, c, d = make(), make(), make(), make()
    assert fuse_map(gmap, views, intr, bg, a) == fuse_map(gmap, views, intr, bg, b, depth="mean") == dict(renders=3, integrations=3, readbacks=0)
    assert torch.equal(torch.stack(a.planes()), torch.stack(b.planes()))
    stats = fuse_map(gmap, views, intr, bg, c, depth="median")
    assert stats == dict(renders=3, integrations=3, readbacks=0) and c.stats == dict(integrations=3, readbacks=0)
    assert fuse_map(gmap, views, intr, bg, d, depth="median", max_std=0.05) == stats and d.stats == c.stats
    acc = {}
    for name, vol in (("mean", a), ("median", c), ("median, max_std 0.05", d)):
        mesh = vol.extract()
        assert mesh.vertices.shape[0] > 0 and mesh.triangles.shape[0] > 0, name
        acc[name] = float(room_surface_distance(mesh.vertices).mean())
        print(f"fuse_map depth={name}: {mesh.vertices.shape[0]} vertices, accuracy_mean_m {acc[name]:.5f}")
        assert math.isfinite(acc[name])
    assert float(c.planes()[1].max()) >= 2.0 and bool((c.planes()[0] < 0).any())
    assert not torch.equal(torch.stack(a.planes()), torch.stack(c.planes()))          # it is another depth
    assert float(d.planes()[1].sum()) <= float(c.planes()[1].sum())                   # the spread gate only removes pixels
    for p in gmap.params():
        assert p.grad is None                                                         # the table-keeping forward leaves no gradient behind


def test_eval_geometry_on_the_room(native_lib, room_map):
    from monogs_amd import eval_geometry
    from monogs_amd.gaussian_optim import activate
    from monogs_amd.mesh_render import MeshRenderer
    from monogs_amd.renderer import render
    from monogs_amd.sequences import room_mesh
    gmap, frs, intr = room_map
    bg = torch.zeros(3, device=DEV)
    views = frs[:3]
    gt = room_mesh(DEV)
    out = eval_geometry(gmap, views, intr, bg, gt_mesh=gt)
    print(f"eval_geometry (mesh): {out}")
    assert {"depth_l1_mean_m", "depth_l1_median_m", "normal_deg_mean", "normal_deg_median", "pixels"} <= set(out)
    assert out["readbacks"] == 1 and out["views"] == 3
    for k in ("depth_l1_mean_m", "depth_l1_median_m", "normal_deg_mean", "normal_deg_median"):
        assert math.isfinite(out[k]) and out[k] >= 0, k
    assert 0 < out["pixels"]["depth_median"] <= out["pixels"]["depth_mean"] and out["pixels"]["normal_mean"] > 0
    assert 0 <= out["normal_deg_mean"] <= 180 and 0 <= out["normal_deg_median"] <= 180
    # depth_l1_mean_m restated in torch
    mr = MeshRenderer(intr, DEV)
    total = torch.zeros((), dtype=torch.float64, device=DEV)
    count = 0
    with torch.no_grad():
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
        for vp in views:
            pkg = render(vp, intr, gmap._xyz.detach(), rot, scales3, opac, gmap._rgb.detach(), bg)
            g = mr.render(gt, vp)["depth"]
            seen = (g > 0) & (pkg["opacity"][0] >= 0.9)
            total += ((pkg["depth"][0] / pkg["opacity"][0])[seen] - g[seen]).abs().double().sum()
            count += int(seen.sum())
    assert count == out["pixels"]["depth_mean"]
    assert abs(out["depth_l1_mean_m"] - float(total) / count) <= 1e-6
    # the viewpoint's own depth as the ground truth
    own = eval_geometry(gmap, views, intr, bg)
    print(f"eval_geometry (frame depth): {own}")
    assert own["readbacks"] == 1 and math.isfinite(own["depth_l1_median_m"]) and abs(own["depth_l1_mean_m"] - out["depth_l1_mean_m"]) < 0.01
