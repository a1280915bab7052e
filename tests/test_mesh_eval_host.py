"""Reconstruction evaluation without a GPU: the ABI and its argument refusals, the mesh PLY reader on quad and uint files, the room's
ground-truth mesh against the room's closed-form distance, and the float64 mirror (tests/mesh_eval_mirror.py) on meshes with a known
answer."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import mesh_eval_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mgs_nn_grid_min", "mgs_nn_scratch_bytes", "mgs_nn_dist2", "mgs_mesh_sample_scratch_bytes", "mgs_mesh_sample",
                "mgs_mesh_mark_seen", "mgs_recon_metrics_scratch_bytes", "mgs_recon_metrics")


def test_abi_version_and_symbols(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 24
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(native_lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        args = [a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[name][1]), (name, args)
    # every symbol the new unit exports is declared, and nothing else of it is exported
    src = open(os.path.join(ROOT, "monogs_amd", "csrc", "mesheval.hip")).read()
    exported = set(re.findall(r"^(?:int|size_t|int32_t) (mgs_\w+)\(", src, flags=re.M))
    assert exported == set(ENTRY_POINTS), exported
    for flag, value in (("MGS_NN_FORCE_ALL_PAIRS", 1), ("MGS_NN_FORCE_MORTON", 2), ("MGS_RECON_MAX_THRESHOLDS", 8)):
        assert re.search(r"#define %s %d\b" % (flag, value), text), flag
    from monogs_amd import mesh_eval
    assert (mesh_eval.NN_FORCE_ALL_PAIRS, mesh_eval.NN_FORCE_MORTON) == (1, 2)
    assert "mesheval.hip" in open(os.path.join(ROOT, "monogs_amd", "csrc", "Makefile")).read()


def test_bad_arguments_are_refused_before_any_launch(native_lib):
    L, p = native_lib, 0x1000              # non-NULL and never dereferenced: the refusals come before any launch
    err = lambda: L.mgs_last_error()  # noqa: E731
    assert L.mgs_nn_dist2(-1, 4, p, p, 0, p, None, p, None) == 1 and b"negative" in err()
    assert L.mgs_nn_dist2(4, (1 << 30) + 1, p, p, 0, p, None, p, None) == 1 and b"2^30" in err()
    assert L.mgs_nn_dist2(4, 4, p, p, 4, p, None, p, None) == 1 and b"unknown flags" in err()
    assert L.mgs_nn_dist2(4, 4, p, p, 3, p, None, p, None) == 1 and b"both paths" in err()
    assert L.mgs_nn_dist2(4, 4, None, p, 0, p, None, p, None) == 1 and b"non-NULL" in err()
    assert L.mgs_nn_dist2(4, 4, p, None, 0, p, None, p, None) == 1
    assert L.mgs_nn_dist2(4, 4, p, p, 0, None, None, p, None) == 1
    assert L.mgs_nn_dist2(4, 4, p, p, 2, p, None, None, None) == 1 and b"scratch" in err()
    assert L.mgs_nn_dist2(0, 4, None, None, 0, None, None, None, None) == 0            # Q == 0: a no-op
    assert L.mgs_mesh_sample(0, 4, p, p, None, 8, 0, p, None, None, p, p, None) == 1 and b"vertices and triangles" in err()
    assert L.mgs_mesh_sample(4, 0, p, p, None, 8, 0, p, None, None, p, p, None) == 1
    assert L.mgs_mesh_sample(4, 4, p, p, None, -1, 0, p, None, None, p, p, None) == 1 and b"N must not" in err()
    for k in (2, 3, 7, 10, 11):            # vertices, triangles, points, status, scratch
        args = [4, 4, p, p, None, 8, 0, p, None, None, p, p, None]
        args[k] = None
        assert L.mgs_mesh_sample(*args) == 1 and b"non-NULL" in err(), k
    assert L.mgs_mesh_mark_seen(-1, p, p, 16, 16, 1.0, 1.0, 8.0, 8.0, None, 0.0, 0.0, 0.0, p, None) == 1
    assert L.mgs_mesh_mark_seen(4, p, p, 0, 16, 1.0, 1.0, 8.0, 8.0, None, 0.0, 0.0, 0.0, p, None) == 1 and b"image size" in err()
    assert L.mgs_mesh_mark_seen(4, p, p, 16, 16, 0.0, 1.0, 8.0, 8.0, None, 0.0, 0.0, 0.0, p, None) == 1 and b"fx and fy" in err()
    assert L.mgs_mesh_mark_seen(4, None, p, 16, 16, 1.0, 1.0, 8.0, 8.0, None, 0.0, 0.0, 0.0, p, None) == 1
    assert L.mgs_mesh_mark_seen(4, p, p, 16, 16, 1.0, 1.0, 8.0, 8.0, None, 0.0, 0.0, 0.0, None, None) == 1
    assert L.mgs_mesh_mark_seen(0, None, None, 16, 16, 1.0, 1.0, 8.0, 8.0, None, 0.0, 0.0, 0.0, None, None) == 0
    thr = (C.c_float * 8)(*([0.05] * 8))
    assert L.mgs_recon_metrics(4, p, 9, thr, p, p, None) == 1 and b"K <= 8" in err()
    assert L.mgs_recon_metrics(-1, p, 1, thr, p, p, None) == 1
    assert L.mgs_recon_metrics(4, None, 1, thr, p, p, None) == 1 and b"non-NULL" in err()
    assert L.mgs_recon_metrics(4, p, 1, thr, None, p, None) == 1
    assert L.mgs_recon_metrics(4, p, 1, thr, p, None, None) == 1


def test_scratch_sizes_are_pure_and_monotone(native_lib):
    f = native_lib.mgs_nn_scratch_bytes
    assert f(0, 100) == f(100, 0) == f(-1, -1) == 256
    last = 0
    for n in (1, 63, 64, 65, 1000, 6143, 6144, 200_000):
        b = f(n, n)
        assert b == f(n, n) and b >= last and b >= 2 * n * (4 * 4 + 16)        # per set: two code + two index arrays, the sorted points
        assert f(n, n + 1) >= b and f(n + 1, n) >= b
        last = b
    assert f(200_000, 200_000) < 64 << 20
    g = native_lib.mgs_mesh_sample_scratch_bytes
    assert g(1) == g(2048) < g(2049) and g(70_000) >= 70_000 * 8 and g(-5) == g(0)
    assert native_lib.mgs_recon_metrics_scratch_bytes() >= 256 * 10 * 8
    assert native_lib.mgs_nn_grid_min() == 6144


def test_cpu_tensors_are_refused():
    from monogs_amd import mesh_eval as ME
    from monogs_amd.tsdf import TriangleMesh
    pts = torch.zeros(10, 3)
    mesh = TriangleMesh(pts, torch.zeros(2, 3, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ME.nearest_distance(pts, pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ME.sample_mesh(mesh, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ME.seen_vertices(mesh, [], None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ME.recon_metrics(torch.zeros(4), [0.05])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ME.eval_reconstruction(mesh, mesh, n_samples=10)
    import monogs_amd
    assert monogs_amd.eval_reconstruction is ME.eval_reconstruction and monogs_amd.nearest_distance is ME.nearest_distance
    src = open(os.path.join(ROOT, "monogs_amd", "mesh_eval.py")).read()
    assert not re.search(r"^\s*(from|import)\s+\S*(slam_harness|mapping)\b", src, flags=re.M)


# ---- the PLY reader ----------------------------------------------------------------------------------------------------------------
VERTS = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.5), (1.0, 1.5, 0.0), (0.0, 1.0, -2.0), (2.0, 2.0, 2.0)]


def _write_ply(path, index_type, faces):
    head = ("ply\nformat binary_little_endian 1.0\ncomment hand-written\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nelement face %d\nproperty list uchar %s vertex_indices\nend_header\n" % (len(VERTS), len(faces), index_type))
    body = b"".join(struct.pack("<3f", *v) for v in VERTS)
    for f in faces:
        body += struct.pack("<B", len(f)) + struct.pack("<%d%s" % (len(f), "I" if index_type == "uint" else "i"), *f)
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii") + body)


def test_load_mesh_ply_reads_quads_and_uint_indices(tmp_path):
    from monogs_amd.ply_io import load_mesh_ply
    p = str(tmp_path / "quads.ply")
    _write_ply(p, "uint", [(0, 1, 2, 3), (1, 4, 2, 0)])                        # how Replica's mesh.ply comes
    m = load_mesh_ply(p)
    assert m.triangles.dtype == torch.int32 and m.vertices.dtype == torch.float32 and m.colors is None
    assert m.triangles.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2], [1, 2, 0]]
    assert torch.equal(m.vertices, torch.tensor(VERTS))
    p = str(tmp_path / "uint.ply")
    _write_ply(p, "uint", [(0, 1, 2), (4, 3, 1)])
    assert load_mesh_ply(p).triangles.tolist() == [[0, 1, 2], [4, 3, 1]]
    p = str(tmp_path / "mixed.ply")
    _write_ply(p, "int", [(0, 1, 2), (0, 1, 2, 3), (4, 3, 1)])
    assert load_mesh_ply(p).triangles.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [4, 3, 1]]
    p = str(tmp_path / "five.ply")
    _write_ply(p, "int", [(0, 1, 2, 3, 4)])
    with pytest.raises(ValueError, match="three or four"):
        load_mesh_ply(p)
    p = str(tmp_path / "huge.ply")
    _write_ply(p, "uint", [(0, 1, 0x80000000)])
    with pytest.raises(ValueError, match="int32"):
        load_mesh_ply(p)


def test_save_mesh_ply_round_trip_is_unchanged(tmp_path):
    from monogs_amd.ply_io import load_mesh_ply, save_mesh_ply
    from monogs_amd.tsdf import TriangleMesh
    v = torch.tensor(VERTS)
    t = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 4]], dtype=torch.int32)
    col = torch.tensor([[0.0, 0.5, 1.0], [0.2, 0.4, 0.6], [1.0, 1.0, 0.0], [0.1, 0.9, 0.3], [0.5, 0.5, 0.5]])
    for name, mesh in (("c", TriangleMesh(v, t, col)), ("n", TriangleMesh(v, t, None)),
                       ("e", TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), None))):
        path = str(tmp_path / f"{name}.ply")
        save_mesh_ply(path, mesh)
        back = load_mesh_ply(path)
        assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.triangles, mesh.triangles)
        assert back.triangles.dtype == torch.int32 and back.triangles.shape[1] == 3 and (back.colors is None) == (mesh.colors is None)
        if mesh.colors is not None:
            assert torch.allclose(back.colors, torch.floor(mesh.colors * 255 + 0.5) / 255, atol=1e-7)


# ---- the room's ground-truth mesh --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_edge", [0.1, 0.37])
def test_room_mesh_lies_on_the_rooms_surfaces(max_edge):
    from monogs_amd.sequences import room_mesh, room_rectangles, room_surface_distance
    m = room_mesh("cpu", max_edge=max_edge, dtype=torch.float64)
    v, t = m.vertices, m.triangles.long()
    assert v.dtype == torch.float64 and m.triangles.dtype == torch.int32 and m.colors is None
    assert float(room_surface_distance(v).abs().max()) <= 1e-12
    assert int(t.min()) == 0 and int(t.max()) == v.shape[0] - 1 and len(torch.unique(t)) == v.shape[0]
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    edges = torch.cat([(b - a).norm(dim=1), (c - b).norm(dim=1), (a - c).norm(dim=1)])
    assert float(edges.max()) <= max_edge + 1e-12 and float(edges.max()) > 0.5 * max_edge
    area = float(0.5 * torch.cross(b - a, c - a, dim=1).norm(dim=1).sum())
    rects = room_rectangles()
    want = sum((ra[2] - ra[1]) * (rb[2] - rb[1]) for _, _, ra, rb in rects)
    assert len(rects) == 6 * 5 and abs(area - want) <= 1e-9 * want, (area, want)
    # the centroids lie on the surfaces too (a triangle does not bridge two rectangles), and the default is float32
    assert float(room_surface_distance((a + b + c) / 3).abs().max()) <= 1e-12
    assert room_mesh("cpu").vertices.dtype == torch.float32


# ---- the mirror against closed forms -----------------------------------------------------------------------------------------------
def _square(z, n=4):
    """A unit square at height z, diced n x n (vertices, triangles)."""
    g = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v00 = (i * (n + 1) + j).ravel()
    t = np.concatenate([np.stack([v00, v00 + n + 1, v00 + n + 2], 1), np.stack([v00, v00 + n + 2, v00 + 1], 1)])
    return v, t.astype(np.int32)


def _covering_radius(v, t, n, seed):
    """How far a point of the mesh can lie from the nearest of its n samples, measured from a 16x denser sample."""
    p, _, _ = M.sample(v, t, n, seed)
    dense, _, _ = M.sample(v, t, 16 * n, seed + 100)
    return float(cKDTree(p).query(dense)[0].max())


def test_mirror_on_two_parallel_squares():
    n, h = 2000, 0.25
    (va, ta), (vb, tb) = _square(0.0), _square(h, n=5)
    fig = M.eval_meshes(va, ta, vb, tb, n, threshold=0.3, seed=4)
    rho = max(_covering_radius(va, ta, n, 4), _covering_radius(vb, tb, n, 5))
    hi = math.sqrt(h * h + rho * rho)
    print(f"parallel squares: accuracy {fig['accuracy_m']:.5f} completion {fig['completion_m']:.5f} in [{h}, {hi:.5f}] (rho {rho:.4f})")
    assert 0 < rho < 0.08
    assert h <= fig["accuracy_m"] <= hi and h <= fig["completion_m"] <= hi
    assert abs(fig["chamfer_l1_m"] - 0.5 * (fig["accuracy_m"] + fig["completion_m"])) < 1e-15
    assert fig["completion_ratio"] == fig["recall"] == 1.0 and fig["precision"] == 1.0 and fig["fscore"] == 1.0
    assert abs(fig["rec_area_m2"] - 1.0) < 1e-6 and abs(fig["gt_area_m2"] - 1.0) < 1e-6
    tight = M.eval_meshes(va, ta, vb, tb, n, threshold=h, seed=4)           # nothing is strictly nearer than h
    assert tight["precision"] == tight["recall"] == tight["fscore"] == 0.0
    same = M.eval_meshes(va, ta, va, ta, n, threshold=0.3, seed=4)
    assert 0 < same["accuracy_m"] <= rho and 0 < same["completion_m"] <= rho


def test_mirror_sampling_rule():
    v, t = _square(0.0, n=3)
    t = np.concatenate([t, [[0, 0, 5], [2, 2, 2]]]).astype(np.int32)           # two zero-area triangles at the end
    keep = np.ones(len(t), np.uint8)
    keep[[1, 4]] = 0
    n = 1800
    p, tri, area = M.sample(v, t, n, 9, keep)
    assert not np.isin(tri, [1, 4, len(t) - 2, len(t) - 1]).any()
    assert abs(area - (18 - 2) / 18) < 1e-6
    counts = np.bincount(tri, minlength=len(t))
    kept = np.nonzero(keep[:-2])[0]
    assert (np.abs(counts[kept] - n / 16) <= 2).all()                          # stratified: fewer than 2 off
    assert (tri[1:] >= tri[:-1]).all()                                         # the strata run through the triangles in order
    u = M.uniforms(9, n)
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.02 and not np.array_equal(u, M.uniforms(10, n))
    assert len(np.unique(u)) > 0.99 * u.size
    assert p[:, 2].max() == 0 and p[:, :2].min() >= 0 and p[:, :2].max() <= 1
    s = M.area_scale(v, len(t))
    assert math.frexp(s)[0] == 0.5 and len(t) * 0.5 * 2.0 * s < 2 ** 60       # a power of two; T x the largest possible area fits


def test_mirror_metrics_and_visibility():
    d2 = np.array([0.0, 0.0025, 0.01, np.inf, 4.0], np.float32)
    m = M.metrics(d2, [0.04, 0.11, 10.0])
    assert m[1] == 4 and abs(m[0] - (0.05 + 0.1 + 2.0)) < 1e-7 and m[2:].tolist() == [1.0, 3.0, 4.0]
    v = np.array([[0, 0, 2.0], [0, 0, -1.0], [5.0, 0, 2.0], [0, 0, 4.0], [0.1, 0.1, 2.0]])
    depth = np.full((16, 16), 3.0)
    depth[9, 9] = 0.0
    ok, _, _ = M.seen(v, np.eye(3), np.zeros(3), 10.0, 10.0, 8.0, 8.0, 16, 16)
    assert ok.tolist() == [True, False, False, True, True]
    ok, _, _ = M.seen(v, np.eye(3), np.zeros(3), 10.0, 10.0, 8.0, 8.0, 16, 16, depth=depth, depth_max=3.5)
    assert ok.tolist() == [True, False, False, False, True]
    v[4] = [0.25, 0.25, 2.0]                                              # pixel (9, 9)
    ok, _, _ = M.seen(v, np.eye(3), np.zeros(3), 10.0, 10.0, 8.0, 8.0, 16, 16, depth=depth)
    assert ok.tolist() == [True, False, False, False, False]               # the fourth is occluded, the fifth falls on the depth hole
