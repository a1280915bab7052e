"""Reconstruction evaluation on the device (csrc/mesheval.hip, monogs_amd/mesh_eval.py) against the float64 mirror of the
specification (tests/mesh_eval_mirror.py) and scipy's cKDTree.

Tolerances.  Nearest neighbour: |d2 - ref| <= 1e-6 ref + 1e-6 m with m = (largest coordinate magnitude)^2 x 2^-24 -- three float32
subtractions and an fma chain carry at most about 8 x 2^-24 relative error, 1e-6 is twice that; both paths and two calls agree bit
for bit, and the reported index reproduces d2 bit for bit.  Sampling: barycentric coordinates in [-1e-5, 1 + 1e-5], plane distance <=
1e-5 of the longest edge, per-triangle counts within 3 of N a_i / A (a stratified draw is fewer than 2 off in exact arithmetic, one
more for a boundary moved by float32 area rounding).  Cull: equal to the mirror wherever the projection is more than 1e-3 px from a
pixel border and the depth margin exceeds 1e-4 m.  Metrics: sums to 1e-12 relative, counts exactly."""
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import mesh_eval_mirror as M
import tsdf_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID_MIN = 6144
NN_SIZES = [(1, 1), (64, 1), (1, 65), (63, 64), (65, 63), (1000, 1000), (257, GRID_MIN - 1), (257, GRID_MIN), (257, GRID_MIN + 1),
            (20_000, 300), (300, 20_000)]
NN_CASES = ("cube", "clusters", "plane", "line", "duplicates", "identical", "offset")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _nn_case(name, Q, P, rng):
    """(queries [Q,3], targets [P,3]) float32."""
    q = rng.uniform(-1, 1, (Q, 3))
    t = rng.uniform(-1, 1, (P, 3))
    if name == "clusters":                      # half the targets 100 units away, every query in the near cluster
        t = t * 0.5
        t[P // 2:, 0] += 100.0
        q = q * 0.5
    elif name == "plane":
        t[:, 2] = 0.25
    elif name == "line":
        t[:, 1], t[:, 2] = -0.5, 0.25
    elif name == "duplicates":                  # every target twice (an odd P: the last one once)
        h = (P + 1) // 2
        t = np.concatenate([t[:h], t[:P - h]])
    elif name == "identical":
        q = t[np.arange(Q) % P]
    elif name == "offset":
        q, t = q + 1000.0, t + 1000.0
    return q.astype(np.float32), t.astype(np.float32)


def _pair_d2_f32(c, q):
    """The pair formula fma(dz, dz, fma(dy, dy, dx dx)) on float32 tensors, each step rounded once (products of float32 are exact in
    float64)."""
    d = (c - q).double()
    s = (d[..., 0] * d[..., 0]).float().double()
    s = (d[..., 1] * d[..., 1] + s).float().double()
    return (d[..., 2] * d[..., 2] + s).float()


@pytest.mark.parametrize("Q, P", NN_SIZES)
def test_nearest_distance(native_lib, Q, P):
    from monogs_amd import mesh_eval as ME
    assert ME.nn_grid_min() == GRID_MIN
    rng = np.random.default_rng(1000 * Q + P)
    for name in NN_CASES:
        qn, tn = _nn_case(name, Q, P, rng)
        q, t = _dev(qn), _dev(tn)
        da, ia = ME.nearest_distance(q, t, want_index=True, path="all_pairs")
        dm, im = ME.nearest_distance(q, t, want_index=True, path="morton")
        dm2, im2 = ME.nearest_distance(q, t, want_index=True, path="morton")
        dd = ME.nearest_distance(q, t)                                              # the default path, without the index
        assert torch.equal(da.view(torch.int32), dm.view(torch.int32)) and torch.equal(ia, im), name
        assert torch.equal(dm.view(torch.int32), dm2.view(torch.int32)) and torch.equal(im, im2), name
        assert torch.equal(dd.view(torch.int32), da.view(torch.int32)), name
        ref = M.nn_tree(qn, tn)
        m = float(max(np.abs(qn).max(), np.abs(tn).max())) ** 2 * 2.0 ** -24
        err = np.abs(da.cpu().numpy().astype(np.float64) - ref)
        worst = float((err - 1e-6 * ref).max())
        print(f"{name} {Q}x{P}: worst |d2 - ref| - 1e-6 ref = {worst:.3e} (allowed {1e-6 * m:.3e})")
        assert worst <= 1e-6 * m, name
        assert int(ia.min()) >= 0 and int(ia.max()) < P
        again = _pair_d2_f32(t[ia.long()], q)
        assert torch.equal(again.view(torch.int32), da.view(torch.int32)), name     # the index attains the float32 minimum
        if Q * P <= 1_100_000:                                                      # ... and is the smallest that does
            full = _pair_d2_f32(t[None, :, :], q[:, None, :])
            first = (full == full.min(dim=1, keepdim=True).values).int().argmax(dim=1)
            assert torch.equal(first.int(), ia), name
        if name == "duplicates" and P > 1:
            assert int(ia.max()) < (P + 1) // 2
        if name == "identical":
            assert not da.any() and torch.equal(ia.long(), torch.arange(Q, device=DEV) % P)


def test_nearest_distance_without_targets_or_queries(native_lib):
    from monogs_amd import mesh_eval as ME
    q = torch.rand(70, 3, device=DEV)
    none = torch.zeros(0, 3, device=DEV)
    for path in (None, "all_pairs", "morton"):
        d2, idx = ME.nearest_distance(q, none, want_index=True, path=path)
        assert torch.isinf(d2).all() and (d2 > 0).all() and (idx == -1).all()
        d2, idx = ME.nearest_distance(none, q, want_index=True, path=path)
        assert d2.shape == (0,) and idx.shape == (0,)
    with pytest.raises(RuntimeError, match=r"\[N,3\]"):
        ME.nearest_distance(torch.rand(5, 2, device=DEV), q)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------
def _sample_meshes():
    rng = np.random.default_rng(7)
    out = {}
    out["one"] = (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.1, 0.9]]), np.array([[0, 1, 2]]), None)
    v = rng.uniform(-1, 1, (40, 3))
    out["65"] = (v, np.stack([rng.permutation(40)[:3] for _ in range(65)]), None)
    # a strip of 24 triangles between two rails whose width jumps by 1e6: area ratios of 1e6
    xs = np.arange(13, dtype=np.float64)
    w = np.where(xs < 6, 1e-3, 1e3)
    v = np.concatenate([np.stack([xs, np.zeros(13), np.zeros(13)], 1), np.stack([xs, w, np.zeros(13)], 1)])
    i = np.arange(12)
    out["strip"] = (v, np.concatenate([np.stack([i, i + 1, i + 14], 1), np.stack([i, i + 14, i + 13], 1)]), None)
    v = rng.uniform(-1, 1, (30, 3))
    t = np.stack([rng.permutation(30)[:3] for _ in range(50)])
    t[::7, 2] = t[::7, 1]                                                              # zero area: a repeated vertex
    v[5] = v[6]
    t[3] = [5, 6, 9]                                                                   # zero area: coincident vertices
    keep = (rng.random(50) < 0.6).astype(np.uint8)
    keep[0] = 1
    keep[1] = 1
    out["zero_and_keep"] = (v, t, keep)
    return out


def _check_samples(name, v, t, keep, n, points, tri, area):
    v64 = v.astype(np.float32).astype(np.float64)
    a, b, c = v64[t[:, 0]], v64[t[:, 1]], v64[t[:, 2]]
    ar = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    if keep is not None:
        ar = np.where(keep != 0, ar, 0.0)
    assert tri.min() >= 0 and tri.max() < len(t)
    assert (ar[tri] > 0).all(), name                                                   # never a zero-area or masked triangle
    assert abs(area - ar.sum()) <= 1e-5 * ar.sum(), (name, area, ar.sum())
    A, B, C, p = a[tri], b[tri], c[tri], points.astype(np.float64)
    e0, e1, d = B - A, C - A, p - A
    nrm = np.cross(e0, e1)
    nn = (nrm * nrm).sum(1)
    w1 = (np.cross(d, e1) * nrm).sum(1) / nn
    w2 = (np.cross(e0, d) * nrm).sum(1) / nn
    longest = np.maximum(np.maximum(np.linalg.norm(e0, axis=1), np.linalg.norm(e1, axis=1)), np.linalg.norm(C - B, axis=1))
    plane = np.abs((d * nrm).sum(1)) / np.sqrt(nn)
    for w in (w1, w2, 1 - w1 - w2):
        assert w.min() >= -1e-5 and w.max() <= 1 + 1e-5, (name, n, w.min(), w.max())
    assert (plane <= 1e-5 * longest).all(), (name, n, float((plane / longest).max()))
    counts = np.bincount(tri, minlength=len(t))
    off = np.abs(counts - n * ar / ar.sum())
    print(f"{name} N={n}: worst count error {off.max():.3f}, worst barycentric excess {max(-w1.min(), -w2.min(), (w1 + w2).max() - 1):.2e}")
    assert off.max() <= 3, (name, n, off.max())


@pytest.mark.parametrize("name", ["one", "65", "strip", "zero_and_keep", "room"])
def test_sample_mesh(native_lib, name):
    from monogs_amd import mesh_eval as ME
    from monogs_amd.sequences import room_mesh
    from monogs_amd.tsdf import TriangleMesh
    if name == "room":
        mesh = room_mesh(DEV)
        v, t, keep = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), None
    else:
        v, t, keep = _sample_meshes()[name]
        mesh = TriangleMesh(_dev(v, torch.float32), _dev(t, torch.int32), None)
    kd = None if keep is None else _dev(keep)
    for n in (1, 64, 1000, 20_000):
        p, tri, area = ME.sample_mesh(mesh, n, seed=3, keep=kd, want_triangles=True)
        assert p.shape == (n, 3) and tri.shape == (n,) and tri.dtype == torch.int32
        _check_samples(name, v, t, keep, n, p.cpu().numpy(), tri.cpu().numpy(), area)
        p2, tri2, area2 = ME.sample_mesh(mesh, n, seed=3, keep=kd, want_triangles=True)
        assert torch.equal(p.view(torch.int32), p2.view(torch.int32)) and torch.equal(tri, tri2) and area == area2
        p3 = ME.sample_mesh(mesh, n, seed=4, keep=kd)
        assert not torch.equal(p, p3)
        if n == 1000:                                                                  # the mirror's rule picks the same strata
            pm, trim, aream = M.sample(v, t, n, 3, keep)
            same = trim == tri.cpu().numpy()
            assert same.mean() >= 0.99 and abs(aream - area) <= 1e-6 * area, (name, same.mean())
            assert np.abs(pm[same] - p.cpu().numpy()[same]).max() <= 1e-5 * max(1.0, np.abs(v).max())


def test_sample_mesh_refuses_bad_meshes(native_lib):
    from monogs_amd import _lib, mesh_eval as ME
    from monogs_amd.rasterizer import _stream
    from monogs_amd.tsdf import TriangleMesh
    v = torch.rand(10, 3, device=DEV)
    for bad in (10, -1, 1 << 30):
        t = torch.tensor([[0, 1, 2], [3, bad, 5], [6, 7, 8]], dtype=torch.int32, device=DEV)
        with pytest.raises(Exception, match="outside"):
            ME.sample_mesh(TriangleMesh(v, t, None), 100)
    # nothing is written outside `points`: the raw call into the middle of a buffer of sentinels
    lib = _lib.load()
    t = torch.tensor([[0, 1, 2], [3, 10, 5], [6, 7, 8]], dtype=torch.int32, device=DEV)
    n, guard = 100, 64
    buf = torch.full((guard + 3 * n + guard,), -7.0, device=DEV)
    tri = torch.full((guard + n + guard,), -7, dtype=torch.int32, device=DEV)
    area, status = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(lib.mgs_mesh_sample_scratch_bytes(3), dtype=torch.uint8, device=DEV)
    rc = lib.mgs_mesh_sample(10, 3, v.data_ptr(), t.data_ptr(), None, n, 5, buf.data_ptr() + 4 * guard, tri.data_ptr() + 4 * guard,
                             area.data_ptr(), status.data_ptr(), scratch.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(status) == 1 and float(area) > 0
    assert (buf[:guard] == -7).all() and (buf[-guard:] == -7).all() and (tri[:guard] == -7).all() and (tri[-guard:] == -7).all()
    got = tri[guard:-guard]
    assert ((got == 0) | (got == 2)).all() and (buf[guard:-guard] != -7).all()        # the bad triangle is never chosen
    # no kept area: an error on the host side
    with pytest.raises(Exception, match="no kept area"):
        ME.sample_mesh(TriangleMesh(v, t[:1], None), 10, keep=torch.zeros(1, dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="no kept area"):
        ME.sample_mesh(TriangleMesh(v, torch.tensor([[1, 1, 2]], dtype=torch.int32, device=DEV), None), 10)


# ---- the cull -----------------------------------------------------------------------------------------------------------------------
CULL_INTR = dict(fx=61.3, fy=60.7, cx=39.7, cy=30.3, W=80, H=60)
CUBE_LO, CUBE_HI = np.array([-0.53, -0.41, 2.03]), np.array([0.61, 0.52, 3.11])


def _cube_vertices(n=23):
    """The six faces of the cube, each diced n x n, and three vertices no camera of the test sees: two behind the first camera, one far
    outside its image."""
    out = []
    for ax in range(3):
        a, b = [i for i in range(3) if i != ax]
        A, B = np.meshgrid(np.linspace(CUBE_LO[a], CUBE_HI[a], n), np.linspace(CUBE_LO[b], CUBE_HI[b], n), indexing="ij")
        for side in (CUBE_LO[ax], CUBE_HI[ax]):
            p = np.zeros(A.shape + (3,))
            p[..., a], p[..., b], p[..., ax] = A, B, side
            out.append(p.reshape(-1, 3))
    out.append(np.array([[0.0, 0.0, -1.0], [0.3, 0.2, -0.01], [40.0, 0.0, 2.5]]))
    return np.concatenate(out).astype(np.float32)


def _rot(rx, ry):
    cx, sx, cy, sy = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry)
    return (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(np.float32)


CULL_POSES = [(_rot(0.031, -0.047), np.array([0.013, -0.021, 0.017], np.float32)),
              (_rot(-0.11, 0.52), np.array([-1.31, 0.07, 0.63], np.float32))]


def _cube_depth(R, t, k=CULL_INTR):
    """z-depth image of the cube by ray casting (slab test), 0 where a ray misses: float32."""
    ys, xs = np.mgrid[0:k["H"], 0:k["W"]].astype(np.float64)
    dc = np.stack([(xs + 0.5 - k["cx"]) / k["fx"], (ys + 0.5 - k["cy"]) / k["fy"], np.ones_like(xs)], -1).reshape(-1, 3)
    R64, t64 = R.astype(np.float64), t.astype(np.float64)
    o = -(R64.T @ t64)
    d = dc @ R64
    d = np.where(np.abs(d) < 1e-12, 1e-12, d)
    t1, t2 = (CUBE_LO - o) / d, (CUBE_HI - o) / d
    tn, tf = np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)
    return np.where((tn < tf) & (tn > 1e-3), tn, 0.0).reshape(k["H"], k["W"]).astype(np.float32)


@pytest.mark.parametrize("with_depth", [False, True])
def test_seen_vertices(native_lib, with_depth):
    from monogs_amd import mesh_eval as ME
    from monogs_amd.frames import Intrinsics
    from monogs_amd.tsdf import TriangleMesh
    k = CULL_INTR
    intr = Intrinsics(dict(k), DEV)
    v = _cube_vertices()
    mesh = TriangleMesh(_dev(v), torch.zeros(0, 3, dtype=torch.int32, device=DEV), None)
    depths = [_cube_depth(R, t) for R, t in CULL_POSES] if with_depth else None
    per_view = []
    for n, (R, t) in enumerate(CULL_POSES):
        want, m_px, m_m = M.seen(v, R, t, k["fx"], k["fy"], k["cx"], k["cy"], k["W"], k["H"], None if depths is None else depths[n])
        clear = (m_px > 1e-3) & (m_m > 1e-4)
        assert clear.mean() >= 0.99, clear.mean()                        # (the mirror alone: at most 1 % are too close to call)
        got = ME.seen_vertices(mesh, [(_dev(R), _dev(t))], intr, None if depths is None else [_dev(depths[n])])
        assert got.dtype == torch.bool and got.shape == (len(v),)
        got = got.cpu().numpy()
        print(f"view {n}, depth {with_depth}: {got.sum()} of {len(v)} seen (mirror {want.sum()}), {int((~clear).sum())} too close to call")
        assert (got[clear] == want[clear]).all()
        assert 0.1 < got.mean() < (0.6 if with_depth else 1.0)
        per_view.append(got)
    assert not per_view[0][-3:].any()                                     # behind the first camera, outside its image
    if with_depth:
        assert per_view[0].sum() < 0.5 * len(v)                           # the cube's back faces are occluded
    both = ME.seen_vertices(mesh, [(_dev(R), _dev(t)) for R, t in CULL_POSES], intr, None if depths is None else [_dev(d) for d in depths])
    assert np.array_equal(both.cpu().numpy(), per_view[0] | per_view[1]) and (both.cpu().numpy() >= per_view[0]).all()      # a second view only adds
    if with_depth:
        assert both.sum() > per_view[0].sum()                             # ... and here it does: a side face
    # cull_mesh keeps the triangles with a seen vertex, in their order, and every vertex
    tri = torch.tensor([[0, 1, 2], [len(v) - 1, len(v) - 2, len(v) - 3], [len(v) - 1, 0, 1]], dtype=torch.int32, device=DEV)
    seen0 = torch.from_numpy(per_view[0]).to(DEV)
    culled = ME.cull_mesh(TriangleMesh(mesh.vertices, tri, None), seen0)
    want_rows = [r for r in tri.tolist() if per_view[0][r].any()]
    assert culled.triangles.tolist() == want_rows and culled.vertices is mesh.vertices


# ---- the figures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 100_000])
def test_recon_metrics(native_lib, n):
    from monogs_amd import mesh_eval as ME
    rng = np.random.default_rng(n)
    d2 = (rng.uniform(0, 0.2, n) ** 2).astype(np.float32)
    if n > 1:
        d2[rng.integers(0, n, max(1, n // 50))] = np.inf
    thr = [0.05, 0.01, 0.1, 0.2, 1e-4, 0.15, 0.07, 10.0]
    for K in (8, 1, 0):
        got = ME.recon_metrics(_dev(d2), thr[:K])
        again = ME.recon_metrics(_dev(d2), thr[:K])
        assert got.dtype == torch.float64 and torch.equal(got, again)
        got, want = got.cpu().numpy(), M.metrics(d2, thr[:K])
        assert abs(got[0] - want[0]) <= 1e-12 * want[0] and np.array_equal(got[1:], want[1:]), (got, want)
    allinf = ME.recon_metrics(torch.full((300,), float("inf"), device=DEV), [0.05]).cpu().tolist()
    assert allinf == [0.0, 0.0, 0.0]
    assert ME.recon_metrics(torch.zeros(0, device=DEV), [0.05]).cpu().tolist() == [0.0, 0.0, 0.0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    from monogs_amd.sequences import room_mesh
    from monogs_amd.tsdf import TSDFVolume
    frs, intr = TC.room_frames(DEV)
    frs = frs[:4]
    for f in frs:
        f.update_RT(f.R_gt.clone(), f.T_gt.clone())
    vol = TSDFVolume.for_bounds(TC.ROOM_LO, TC.ROOM_HI, TC.ROOM_VOXEL, DEV, trunc=TC.ROOM_TRUNC)
    for f in frs:
        vol.integrate(f.depth, f.R_gt, f.T_gt, intr, rgb=f.rgb)
    return frs, intr, vol.extract(), room_mesh(DEV)


FIGURES = ("accuracy_m", "completion_m", "completion_ratio", "chamfer_l1_m", "precision", "recall", "fscore")


def test_eval_reconstruction_of_the_fused_room(native_lib, room):
    from monogs_amd import mesh_eval as ME
    from monogs_amd.sequences import room_surface_distance
    frs, intr, rec, gt = room
    n = 20_000
    out = ME.eval_reconstruction(rec, gt, n_samples=n, return_samples=True)
    assert set(out) == set(FIGURES) | {"rec_area_m2", "gt_area_m2", "n_samples", "threshold_m", "readbacks", "rec_samples", "gt_samples",
                                       "rec_d2", "gt_d2"}
    assert out["readbacks"] == 1 and out["n_samples"] == n and out["threshold_m"] == 0.05
    pr, pg = out["rec_samples"].cpu().numpy(), out["gt_samples"].cpu().numpy()
    d = np.sqrt(out["rec_d2"].cpu().numpy().astype(np.float64))
    true = room_surface_distance(torch.from_numpy(pr.astype(np.float64))).abs().numpy()
    assert (d >= true - 1e-5).all(), float((true - d).max())             # the ground-truth samples lie ON the surfaces
    dense = ME.sample_mesh(gt, 4 * n, seed=77).cpu().numpy()
    rho = float(cKDTree(pg).query(dense)[0].max())
    print(f"room: accuracy {out['accuracy_m']:.5f} m, mean true distance {true.mean():.5f} m, covering radius {rho:.4f} m")
    assert -1e-6 <= out["accuracy_m"] - true.mean() <= rho
    want = M.figures(M.nn_tree(pr, pg), M.nn_tree(pg, pr), 0.05)
    for k in FIGURES:
        assert abs(out[k] - want[k]) <= 1e-6, (k, out[k], want[k])
    gt64 = gt.vertices.double()
    t = gt.triangles.long()
    area = float(0.5 * torch.cross(gt64[t[:, 1]] - gt64[t[:, 0]], gt64[t[:, 2]] - gt64[t[:, 0]], dim=1).norm(dim=1).sum())
    assert abs(out["gt_area_m2"] - area) <= 1e-5 * area and out["rec_area_m2"] > 5.0
    # culled by the four frames and their depth, the unseen backs of the boxes and the walls behind the camera no longer count
    culled = ME.eval_reconstruction(rec, gt, n_samples=n, viewpoints=frs, intr=intr, depths=[f.depth for f in frs])
    print(f"room: completion ratio {out['completion_ratio']:.4f} unculled, {culled['completion_ratio']:.4f} culled; "
          f"ground-truth area {out['gt_area_m2']:.2f} -> {culled['gt_area_m2']:.2f} m2; culled figures {[round(culled[k], 5) for k in FIGURES]}")
    assert culled["readbacks"] == 1 and set(culled) == set(out) - {"rec_samples", "gt_samples", "rec_d2", "gt_d2"}
    assert culled["completion_ratio"] > out["completion_ratio"] and culled["gt_area_m2"] < out["gt_area_m2"]
    assert 0 < culled["completion_ratio"] <= 1
    # the keep mask of the culled call is cull_mesh's rule
    seen = ME.seen_vertices(gt, frs, intr, [f.depth for f in frs])
    by_mesh = ME.eval_reconstruction(rec, ME.cull_mesh(gt, seen), n_samples=n)
    assert abs(by_mesh["gt_area_m2"] - culled["gt_area_m2"]) <= 1e-6 * culled["gt_area_m2"]      # (another T: another fixed-point scale)


def test_run_slam_scores_its_mesh(native_lib, tmp_path):
    from monogs_amd.slam_harness import run_slam
    run = dict(n_frames=4, intrinsics=TC.ROOM_INTR, tracking_itr_num=40, mapping_itr_num=30, init_itr_num=300, window_size=4,
               kf_interval=2, scene="room", mesh_voxel=0.04)
    with open(os.path.join(GOLDEN, "run_slam_contract.json")) as f:
        recorded = {k for k in json.load(f)["eager"]["keys"] if "." not in k}
    out = run_slam(mesh_path=str(tmp_path / "a.ply"), mesh_gt="room", mesh_samples=20_000, **run)
    assert set(out) == recorded | {"mesh"}
    today = {"path", "vertices", "triangles", "voxel", "integrate_ms", "extract_ms", "accuracy_mean_m"}
    assert set(out["mesh"]) == today | {"reconstruction"}
    r = out["mesh"]["reconstruction"]
    print(f"run_slam reconstruction: {r}")
    assert set(r) == set(FIGURES) | {"rec_area_m2", "gt_area_m2", "n_samples", "threshold_m", "readbacks"}
    assert all(math.isfinite(float(r[k])) for k in r) and 0 < r["completion_ratio"] <= 1 and r["readbacks"] == 1 and r["n_samples"] == 20_000
    plain = run_slam(mesh_path=str(tmp_path / "b.ply"), **run)
    assert set(plain["mesh"]) == today and set(plain) == recorded | {"mesh"}
