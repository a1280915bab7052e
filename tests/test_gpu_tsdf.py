"""TSDF fusion and mesh extraction on the device (csrc/tsdf.hip, monogs_amd/tsdf.py) against the float64 mirror of the specification
(tests/tsdf_mirror.py) on the inputs of tests/tsdf_cases.py -- a few thousand voxels: a grid whose x is no multiple of the 64-voxel
brick and whose total is no multiple of a workgroup or a scan block, three poses (one with the grid partly behind the camera and
partly outside the image), a weight cap the third frame reaches, a depth_max that cuts, an opacity ramp across opacity_min.

Tolerances.  A float32 kernel may decide a voxel whose margin (tests/tsdf_mirror.py) is below 1e-4 pixels or 1e-5 metres / opacity
units the other way: those are exempt, and tests/test_tsdf_host.py shows their share stays below 2e-3.  Elsewhere the weight is equal
exactly; tsdf within 1e-4 (float32 eps x coordinates <= 8 m x a handful of operations ~ 2e-6 m, over trunc >= 0.04); colour within
1e-5.  Mesh vertices and colours: 1e-6 of the grid's diagonal.  Index buffers: identical."""
import json
import math
import os

import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_mirror as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _intr():
    from monogs_amd.frames import Intrinsics
    return Intrinsics(dict(fx=TC.FX, fy=TC.FY, cx=TC.CX, cy=TC.CY, W=TC.W, H=TC.H), DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _integrate_all(vol, frs, intr, **kw):
    for f in frs:
        vol.integrate(_dev(f["depth"]), _dev(f["R"]), _dev(f["t"]), intr, rgb=_dev(f["rgb"]), opacity=_dev(f["opacity"]),
                      depth_min=TC.DEPTH_MIN, depth_max=f["depth_max"], opacity_min=TC.OPACITY_MIN, **kw)


def _volume(origin, color):
    from monogs_amd.tsdf import TSDFVolume
    return TSDFVolume(origin, TC.S, TC.DIMS, DEV, color=color, trunc=TC.TRUNC, max_weight=TC.MAX_WEIGHT)


def _planes_np(vol):
    return [None if p is None else p.cpu().numpy() for p in vol.planes()]


@pytest.mark.parametrize("opacity", [False, True])
@pytest.mark.parametrize("color", [False, True])
def test_integrate_matches_the_mirror(native_lib, opacity, color):
    frs = TC.frames(opacity, color)
    planes, seen, amb, per = TC.run_mirror(frs, TC.ORIGIN, color)
    vol = _volume(TC.ORIGIN, color)
    assert [tuple(p.shape) for p in vol.planes() if p is not None] == [(19, 20, 37)] * (5 if color else 2)
    _integrate_all(vol, frs, _intr())
    got = _planes_np(vol)
    share = float(amb.mean())
    ok = ~amb
    d_t = np.abs(got[0] - planes[0])[ok].max()
    print(f"opacity {opacity} colour {color}: ambiguous share {share:.2e}, visited {seen.mean():.3f}, weight 2 on {(planes[1] == 2).mean():.3f}, "
          f"max |tsdf - mirror| {d_t:.2e}")
    assert share <= TC.AMBIGUOUS_CAP
    assert (got[1][ok] == planes[1][ok]).all(), int((got[1][ok] != planes[1][ok]).sum())
    assert d_t <= 1e-4
    if color:
        d_c = max(np.abs(got[2 + c] - planes[2 + c])[ok].max() for c in range(3))
        print(f"max |colour - mirror| {d_c:.2e}")
        assert d_c <= 1e-5
    untouched = ok & (planes[1] == 0)
    assert untouched.any()
    assert (got[0][untouched] == 1.0).all() and (got[1][untouched] == 0.0).all()
    for c in range(2, 5 if color else 2):
        assert (got[c][untouched] == 0.0).all()
    assert vol.stats == dict(integrations=3, readbacks=0)


def test_a_frame_without_colour_leaves_the_colour_planes_alone(native_lib):
    vol = _volume(TC.ORIGIN, True)
    _integrate_all(vol, TC.frames(False, False), _intr())
    t, w, r, g, b = vol.planes()
    assert float(w.max()) == TC.MAX_WEIGHT and not r.any() and not g.any() and not b.any()
    vol.reset()
    assert bool((vol.planes()[0] == 1).all()) and not vol.planes()[1].any()


def test_culling_changes_nothing(native_lib):
    frs = TC.frames(True, True)
    planes, seen, amb, per = TC.run_mirror(frs, TC.ORIGIN_CULLED, True)
    intr = _intr()
    runs = []
    for kw in (dict(), dict(), dict(cull=False)):
        vol = _volume(TC.ORIGIN_CULLED, True)
        _integrate_all(vol, frs, intr, **kw)
        runs.append(torch.stack(vol.planes()).clone())
    assert torch.equal(runs[0], runs[1])                        # two runs, bit for bit
    assert torch.equal(runs[0], runs[2])                        # culled and unculled, bit for bit
    touched = (runs[0][1] > 0).cpu().numpy()
    ok = ~amb
    print(f"shifted volume: mirror visits {seen.mean():.3f} of the voxels, device {touched.mean():.3f}; ambiguous {amb.mean():.2e}")
    assert 0 < seen.mean() < 0.25
    assert (touched[ok] == seen[ok]).all()
    assert np.abs(runs[0][0].cpu().numpy() - planes[0])[ok].max() <= 1e-4


def _load_case(c):
    from monogs_amd.tsdf import TSDFVolume
    vol = TSDFVolume(c["origin"], c["s"], c["dims"], DEV, color=c["colors"] is not None)
    p = vol.planes()
    p[0].copy_(_dev(c["tsdf"]))
    p[1].copy_(_dev(c["weight"]))
    if c["colors"] is not None:
        for n in range(3):
            p[2 + n].copy_(_dev(c["colors"][n]))
    return vol


@pytest.mark.parametrize("name", ["sphere", "plane", "unobserved_block", "min_weight_2", "exact_zero", "all_positive"])
def test_extract_matches_the_mirror(native_lib, name):
    from monogs_amd.tsdf import mesh_stats
    c = TC.extract_cases()[name]
    want = TC.mirror_extract(c)
    vol = _load_case(c)
    mesh = vol.extract(min_weight=c["min_weight"])
    assert vol.stats["readbacks"] == 1
    V, T = mesh.vertices.shape[0], mesh.triangles.shape[0]
    assert mesh.vertices.dtype == torch.float32 and mesh.triangles.dtype == torch.int32
    assert (V, T) == (len(want["vertices"]), len(want["triangles"]))
    if name == "all_positive":
        assert V == 0 and T == 0 and mesh.triangles.shape == (0, 3) and mesh.colors is None
        return
    tri = mesh.triangles.cpu().numpy().astype(np.int64)
    assert (tri == want["triangles"]).all()
    assert tri.min() >= 0 and tri.max() < V and len(np.unique(tri)) == V                 # no index >= V, every vertex referenced
    extent = c["s"] * math.sqrt(sum((d - 1) ** 2 for d in c["dims"]))
    dv = np.abs(mesh.vertices.cpu().numpy() - want["vertices"]).max()
    print(f"{name}: V {V} T {T}, max |vertex - mirror| {dv:.2e} (grid diagonal {extent:.3f})")
    assert dv <= 1e-6 * extent
    if c["colors"] is not None:
        dc = np.abs(mesh.colors.cpu().numpy() - want["colors"]).max()
        print(f"max |colour - mirror| {dc:.2e}")
        assert dc <= 1e-6 * extent
    else:
        assert mesh.colors is None
    st = mesh_stats(mesh)
    chk = M.mesh_checks(want["vertices"], want["triangles"])
    assert (st["boundary_edges"], st["non_manifold_edges"]) == (chk["boundary"], chk["non_manifold"])
    if name == "sphere":
        assert st["boundary_edges"] == 0 and st["non_manifold_edges"] == 0
        assert abs(st["volume"] - chk["volume"]) <= 1e-5 * chk["volume"] and st["volume"] > 0
    if name in ("unobserved_block", "min_weight_2"):
        # every triangle lies inside one cell; that cell is valid
        v = mesh.vertices.cpu().numpy().astype(np.float64)
        cen = v[tri].mean(axis=1)
        cell = np.floor((cen - np.asarray(c["origin"], np.float64)) / c["s"]).astype(np.int64)
        assert (cell >= 0).all() and (cell < np.asarray(c["dims"]) - 1).all()
        assert want["valid"][cell[:, 2], cell[:, 1], cell[:, 0]].all() and not want["valid"].all()
    # a second extraction from the same planes: the same mesh, bit for bit
    again = vol.extract(min_weight=c["min_weight"])
    assert torch.equal(again.vertices, mesh.vertices) and torch.equal(again.triangles, mesh.triangles)


@pytest.fixture(scope="module")
def room():
    frs, intr = TC.room_frames(DEV)
    for f in frs:
        f.update_RT(f.R_gt.clone(), f.T_gt.clone())
    return frs, intr


def test_ground_truth_fusion_of_the_room(native_lib, room):
    """Every vertex lies within half a voxel diagonal (+ 1 mm) of the room's true surfaces, but for at most 1 % that sit within the
    truncation distance of a depth discontinuity of some frame (tests/tsdf_cases.py says why the truncation is 2 voxels)."""
    from monogs_amd.tsdf import TSDFVolume, mesh_stats
    frs, intr = room
    vol = TSDFVolume.for_bounds(TC.ROOM_LO, TC.ROOM_HI, TC.ROOM_VOXEL, DEV, trunc=TC.ROOM_TRUNC)
    assert vol.dims == TC.room_dims()
    for f in frs:
        vol.integrate(f.depth, f.R_gt, f.T_gt, intr, rgb=f.rgb)
    mesh = vol.extract()
    fig = TC.check_room_mesh(mesh.vertices.cpu().numpy(), frs, intr)
    assert fig["vertices"] > 50000 and mesh.triangles.shape[0] > 0
    st = mesh_stats(mesh)
    print(f"room mesh: {st}")
    assert st["non_manifold_edges"] == 0 and st["area"] > 20.0
    assert float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0 and float(mesh.colors.mean()) > 0.2


def test_fuse_map_is_render_plus_integrate(native_lib, room):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.gaussian_optim import activate
    from monogs_amd.renderer import render
    from monogs_amd.tsdf import TSDFVolume, fuse_map
    frs, intr = room
    bg = torch.zeros(3, device=DEV)
    gmap = GaussianMap(DEV)
    gmap.extend_from_frame(frs[0], intr, downsample=8, init=True, point_size=1.0)
    gmap._opacity.data.fill_(4.0)                                # opaque splats (0.98): the render's opacity passes opacity_min unmapped
    views = frs[:3]
    make = lambda: TSDFVolume.for_bounds(TC.ROOM_LO, TC.ROOM_HI, 0.08, DEV)  # noqa: E731
    a, b = make(), make()
    stats = fuse_map(gmap, views, intr, bg, a)
    assert stats == dict(renders=3, integrations=3, readbacks=0) and a.stats == dict(integrations=3, readbacks=0)
    with torch.no_grad():
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
        for vp in views:
            pkg = render(vp, intr, gmap._xyz.detach(), rot, scales3, opac, gmap._rgb.detach(), bg)
            b.integrate(pkg["depth"], vp.R, vp.T, intr, rgb=pkg["render"], opacity=pkg["opacity"])
    assert torch.equal(torch.stack(a.planes()), torch.stack(b.planes()))
    assert float(a.planes()[1].max()) >= 2.0 and bool((a.planes()[0] < 0).any())
    # integrate is one launch and no host synchronisation: captured once, replayed twice = two eager calls
    f = frs[1]
    c, d = make(), make()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.integrate(f.depth, f.R_gt, f.T_gt, intr, rgb=f.rgb)
    assert not c.planes()[1].any()                               # capture launches nothing
    graph.replay()
    graph.replay()
    for _ in range(2):
        d.integrate(f.depth, f.R_gt, f.T_gt, intr, rgb=f.rgb)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(c.planes()), torch.stack(d.planes())) and float(d.planes()[1].max()) == 2.0


ROOM_RUN = dict(n_frames=12, intrinsics=TC.ROOM_INTR, tracking_itr_num=100, mapping_itr_num=60, init_itr_num=600, window_size=4,
                kf_interval=2, scene="room")


def test_run_slam_writes_the_mesh_and_keeps_its_keys(native_lib, tmp_path):
    from monogs_amd.ply_io import load_mesh_ply
    from monogs_amd.slam_harness import run_slam
    with open(os.path.join(GOLDEN, "run_slam_contract.json")) as f:
        recorded = {k for k in json.load(f)["eager"]["keys"] if "." not in k}
    path = str(tmp_path / "room.ply")
    out = run_slam(mesh_path=path, mesh_voxel=0.04, **ROOM_RUN)
    assert set(out) == recorded | {"mesh"}
    m = out["mesh"]
    assert set(m) == {"path", "vertices", "triangles", "voxel", "integrate_ms", "extract_ms", "accuracy_mean_m"}
    assert m["path"] == path and m["voxel"] == 0.04 and m["vertices"] > 1000 and m["triangles"] > 1000
    assert m["integrate_ms"] > 0 and m["extract_ms"] > 0 and 0 < m["accuracy_mean_m"] < 0.5
    print(f"run_slam mesh: {m}")
    mesh = load_mesh_ply(path)
    assert mesh.vertices.shape == (m["vertices"], 3) and mesh.triangles.shape == (m["triangles"], 3)
    assert mesh.colors is not None and int(mesh.triangles.max()) < m["vertices"] and int(mesh.triangles.min()) >= 0
    assert set(run_slam(**ROOM_RUN)) == recorded
