"""TSDF fusion and mesh extraction without a GPU: the ABI and its argument refusals, the mesh PLY format, the float64 mirror
(tests/tsdf_mirror.py) on a sphere with a known answer, ``room_surface_distance`` against brute force, and the two claims the GPU
tests lean on -- the share of voxels whose decisions are too close to call in float32 stays below the cap on the inputs of
tests/test_gpu_tsdf.py, and the room mesh of the mirror stays within the room test's bounds."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_and_symbols(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 23
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    for name in ("mgs_tsdf_integrate", "mgs_tsdf_extract_scratch_bytes", "mgs_tsdf_extract_count", "mgs_tsdf_extract_emit"):
        assert name in _lib.SIGNATURES and hasattr(native_lib, name)
    assert C.sizeof(_lib.MgsTsdfVolume) == 7 * 4 + 4 + 5 * 8 and C.sizeof(_lib.MgsTsdfFrame) == 2 * 4 + 4 * 8 + 10 * 4


def _volume(nx=8, ny=8, nz=8, voxel=0.1, planes=5):
    from monogs_amd import _lib
    v = _lib.MgsTsdfVolume()
    v.nx, v.ny, v.nz, v.voxel = nx, ny, nz, voxel
    ptr = [0x1000] * planes + [None] * (5 - planes)          # non-NULL and never dereferenced: the refusals come before any launch
    v.tsdf, v.weight, v.r, v.g, v.b = ptr
    return v


def _frame(trunc=0.4):
    from monogs_amd import _lib
    f = _lib.MgsTsdfFrame()
    f.width, f.height, f.depth, f.viewmatrix = 16, 16, 0x1000, 0x1000
    f.fx = f.fy = 10.0
    f.cx = f.cy = 8.0
    f.trunc, f.depth_min, f.max_weight = trunc, 0.01, 64.0
    return f


@pytest.mark.parametrize("what, vol, text", [
    ("null plane", dict(planes=1), b"tsdf and weight"),
    ("two colour planes", dict(planes=4), b"all three or none"),
    ("zero dimension", dict(nx=0), b"dimensions must be positive"),
    ("negative dimension", dict(nz=-3), b"dimensions must be positive"),
    ("2^31 voxels", dict(nx=2048, ny=1024, nz=1024), b"below 2^31"),
    ("voxel", dict(voxel=0.0), b"voxel edge"),
])
def test_bad_volumes_are_refused_by_every_entry_point(native_lib, what, vol, text):
    v, f = _volume(**vol), _frame()
    assert native_lib.mgs_tsdf_integrate(C.byref(v), C.byref(f), None) == 1 and text in native_lib.mgs_last_error(), what
    assert native_lib.mgs_tsdf_extract_count(C.byref(v), 1.0, 0x1000, 0x1000, None) == 1 and text in native_lib.mgs_last_error()
    assert native_lib.mgs_tsdf_extract_emit(C.byref(v), 0x1000, 0x1000, None, 0x1000, 1, 1, None) == 1
    assert text in native_lib.mgs_last_error()


def test_bad_frames_and_pointers_are_refused(native_lib):
    v = _volume()
    for trunc in (0.0, -0.1, float("nan")):
        f = _frame(trunc)
        assert native_lib.mgs_tsdf_integrate(C.byref(v), C.byref(f), None) == 1 and b"trunc must be positive" in native_lib.mgs_last_error()
    for field, text in (("depth", b"depth and viewmatrix"), ("viewmatrix", b"depth and viewmatrix"), ("width", b"image size"),
                        ("max_weight", b"max_weight"), ("fx", b"fx and fy")):
        f = _frame()
        setattr(f, field, 0)
        assert native_lib.mgs_tsdf_integrate(C.byref(v), C.byref(f), None) == 1 and text in native_lib.mgs_last_error(), field
    assert native_lib.mgs_tsdf_integrate(None, C.byref(_frame()), None) == 1
    assert native_lib.mgs_tsdf_integrate(C.byref(v), None, None) == 1
    assert native_lib.mgs_tsdf_extract_count(C.byref(v), 1.0, None, 0x1000, None) == 1 and b"scratch and counts" in native_lib.mgs_last_error()
    assert native_lib.mgs_tsdf_extract_count(C.byref(v), 1.0, 0x1000, None, None) == 1
    assert native_lib.mgs_tsdf_extract_emit(C.byref(v), None, 0x1000, None, 0x1000, 1, 1, None) == 1
    assert native_lib.mgs_tsdf_extract_emit(C.byref(v), 0x1000, None, None, 0x1000, 1, 1, None) == 1
    assert native_lib.mgs_tsdf_extract_emit(C.byref(v), 0x1000, 0x1000, None, 0x1000, 1 << 31, 1, None) == 1
    assert b"below 2^31" in native_lib.mgs_last_error()
    assert native_lib.mgs_tsdf_extract_emit(C.byref(_volume(planes=2)), 0x1000, 0x1000, 0x1000, 0x1000, 1, 1, None) == 1
    assert b"without colour" in native_lib.mgs_last_error()
    # an empty mesh is nothing to emit: no launch, no error
    assert native_lib.mgs_tsdf_extract_emit(C.byref(v), 0x1000, None, None, None, 0, 0, None) == 0


def test_scratch_bytes_is_pure_and_monotone(native_lib):
    f = native_lib.mgs_tsdf_extract_scratch_bytes
    assert f(0, 4, 4) == f(4, -1, 4) == f(2048, 1024, 1024) == 256
    last = 0
    for n in (1, 2, 7, 37, 64, 65, 128, 301):
        b = f(n, 20, 19)
        assert b == f(n, 20, 19) and b >= last and b >= n * 20 * 19 * 12      # four byte planes + two word planes
        assert f(20, n, 19) <= f(20, n + 1, 19) and f(20, 19, n) <= f(20, 19, n + 1)
        last = b
    assert f(300, 150, 300) < 300 * 150 * 300 * 12 + (1 << 20)


def test_mesh_ply_round_trip(tmp_path):
    from monogs_amd.ply_io import load_mesh_ply, save_mesh_ply
    from monogs_amd.tsdf import TriangleMesh
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.5, 0.0], [0.25, 0.25, -2.0]])
    t = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2]], dtype=torch.int32)
    col = torch.tensor([[0.0, 0.5, 1.0], [0.2, 0.4, 0.6], [1.0, 1.0, 0.0], [1.2, -0.1, 0.3]])
    for name, mesh in (("c", TriangleMesh(v, t, col)), ("n", TriangleMesh(v, t, None)),
                       ("e", TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3))),
                       ("en", TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), None))):
        path = str(tmp_path / f"{name}.ply")
        save_mesh_ply(path, mesh)
        head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"]
        assert "property list uchar int vertex_indices" in head and ("property uchar red" in head) == (mesh.colors is not None)
        back = load_mesh_ply(path)
        assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.triangles, mesh.triangles)
        assert back.triangles.dtype == torch.int32 and back.vertices.dtype == torch.float32
        if mesh.colors is None:
            assert back.colors is None
        else:
            want = torch.floor(mesh.colors.clamp(0, 1) * 255 + 0.5) / 255
            assert torch.allclose(back.colors, want, atol=1e-7)
        n_v, n_f = mesh.vertices.shape[0], mesh.triangles.shape[0]
        assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + n_v * (12 + (3 if mesh.colors is not None else 0)) + n_f * 13


def test_mirror_sphere_is_closed_oriented_and_accurate():
    c = TC.sphere_case()
    s, r = c["s"], c["radius"]
    m = TC.mirror_extract(c)
    chk = M.mesh_checks(m["vertices"], m["triangles"])
    assert chk["closed"] and chk["euler"] == 2 and chk["boundary"] == 0 and chk["non_manifold"] == 0, chk
    exact = 4.0 / 3.0 * math.pi * r ** 3
    assert 0 < chk["volume"] and abs(chk["volume"] - exact) <= 0.05 * exact, (chk["volume"], exact)
    err = np.abs(np.linalg.norm(m["vertices"] - c["centre"], axis=1) - r)
    bound = 1.01 * 3 * s * s / (8 * (r - math.sqrt(3) * s))
    print(f"sphere: {len(m['vertices'])} vertices, {len(m['triangles'])} triangles, volume {chk['volume']:.6f} (exact {exact:.6f}), "
          f"worst radial error {err.max():.3e} (bound {bound:.3e})")
    assert err.max() <= bound
    assert m["triangles"].max() < len(m["vertices"]) and len(np.unique(m["triangles"])) == len(m["vertices"])
    # colours are interpolated with the vertex's own factor: they stay inside the range of the edge's two ends
    assert m["colors"].min() >= 0.0 and m["colors"].max() <= 1.0


def test_mirror_extract_cases_are_consistent():
    for name, c in TC.extract_cases().items():
        m = TC.mirror_extract(c)
        V, T = len(m["vertices"]), len(m["triangles"])
        if name == "all_positive":
            assert V == 0 and T == 0
            continue
        assert V > 0 and T > 0, name
        assert m["triangles"].max() < V and len(np.unique(m["triangles"])) == V, name      # every vertex referenced, none missing
        chk = M.mesh_checks(m["vertices"], m["triangles"])
        assert chk["non_manifold"] == 0, (name, chk)
        if name in ("unobserved_block", "min_weight_2"):
            assert chk["boundary"] > 0, name                                              # the hole has a rim
        lo = np.asarray(c["origin"], np.float64)
        hi = lo + c["s"] * (np.asarray(c["dims"]) - 1)
        assert (m["vertices"] >= lo - 1e-6).all() and (m["vertices"] <= hi + 1e-6).all(), name


def test_room_surface_distance_against_brute_force():
    from monogs_amd.sequences import _ROOM_BOXES, _ROOM_HALF, room_surface_distance
    step = 0.05
    faces = []
    for lo, hi in [((-_ROOM_HALF[0], -_ROOM_HALF[1], -_ROOM_HALF[2]), _ROOM_HALF)] + list(_ROOM_BOXES):
        for ax in range(3):
            a, b = [i for i in range(3) if i != ax]
            ga = np.linspace(lo[a], hi[a], int(round((hi[a] - lo[a]) / step)) + 1)
            gb = np.linspace(lo[b], hi[b], int(round((hi[b] - lo[b]) / step)) + 1)
            A, B = np.meshgrid(ga, gb, indexing="ij")
            for side in (lo[ax], hi[ax]):
                pts = np.zeros(A.shape + (3,))
                pts[..., a], pts[..., b], pts[..., ax] = A, B, side
                faces.append(pts.reshape(-1, 3))
    samples = torch.from_numpy(np.concatenate(faces))
    assert float(room_surface_distance(samples).abs().max()) < 1e-12                       # every face point is on the surface
    rng = np.random.default_rng(3)
    q = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(400, 3)) * np.array([3.4, 1.8, 3.4]))
    brute = torch.cdist(q, samples).min(dim=1).values
    d = room_surface_distance(q)
    # a face sample lies within half a grid diagonal of the closest face point: brute force can only be larger, by at most that
    assert (brute >= d - 1e-9).all() and (brute - d).max() <= step * math.sqrt(2) / 2 + 1e-9, float((brute - d).max())
    assert room_surface_distance(q.float()).dtype == torch.float32


@pytest.mark.parametrize("origin", [TC.ORIGIN, TC.ORIGIN_CULLED])
def test_ambiguous_share_of_the_gpu_inputs_meets_the_cap(origin):
    worst = 0.0
    for opacity in (False, True):
        planes, seen, amb, per = TC.run_mirror(TC.frames(opacity, True), origin, True)
        worst = max(worst, float(amb.mean()))
        if origin == TC.ORIGIN:
            # the inputs exercise what they are meant to: the weight cap, untouched voxels, the third pose's culled parts
            assert planes[1].max() == TC.MAX_WEIGHT and (sum(p.astype(int) for p in per) == 3).any()
            assert 0.2 < seen.mean() < 0.95 and 0.02 < per[2].mean() < 0.8
        else:
            assert 0.0 < seen.mean() < 0.25
    print(f"ambiguous share at origin {origin}: {worst:.2e} (cap {TC.AMBIGUOUS_CAP:.0e})")
    assert worst <= TC.AMBIGUOUS_CAP


def test_room_mesh_of_the_mirror_stays_within_the_room_tests_bounds():
    frs, intr = TC.room_frames("cpu")
    dims = TC.room_dims()
    planes = M.new_planes(dims, color=False)
    for f in frs:
        M.integrate(planes, TC.ROOM_LO, TC.ROOM_VOXEL, dims, f.depth.numpy(), f.R_gt.numpy(), f.T_gt.numpy(), intr.fx, intr.fy, intr.cx,
                    intr.cy, TC.ROOM_TRUNC)
    m = M.extract(planes[0], planes[1], TC.ROOM_LO, TC.ROOM_VOXEL, dims)
    fig = TC.check_room_mesh(m["vertices"], frs, intr)
    assert fig["vertices"] > 50000


def test_module_stands_apart_from_the_run_loops():
    """monogs_amd.tsdf is usable from an evaluation script: it imports neither the harness nor the mapper."""
    src = open(os.path.join(ROOT, "monogs_amd", "tsdf.py")).read()
    assert not re.search(r"^\s*(from|import)\s+\S*(slam_harness|mapping)\b", src, flags=re.M)
    import monogs_amd
    assert monogs_amd.TSDFVolume.__module__ == "monogs_amd.tsdf" and callable(monogs_amd.fuse_map)
