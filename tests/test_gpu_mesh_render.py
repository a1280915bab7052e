"""Mesh rendering and Depth L1 on the device (csrc/mesh_render.hip, csrc/metrics.hip, monogs_amd/mesh_render.py) against the float64
mirror of the specification (tests/mesh_render_mirror.py) and, for the room, against the closed form of ``raycast_room``.

Tolerances (tests/mesh_render_cases.py; measured by tests/test_mesh_render_host.py), at the pixels the mirror does not call ambiguous:
hit / no-hit equal to the mirror's; depth within DEPTH_RTOL = 4 x 3.5e-6 relative; colour within COLOR_ATOL = 4 x 1.5e-5; the reported
id a triangle the mirror's grown test accepts at that pixel at a depth within DEPTH_RTOL of the image's; label == face_labels[tri_id]
exactly, everywhere.  Against ``raycast_room``: depth within DEPTH_RTOL x depth + 1e-5 m, ids equal.  Depth L1 sums: 1e-12 relative."""
import math

import numpy as np
import pytest
import torch

import mesh_render_cases as MC
import mesh_render_mirror as M
import tsdf_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _intr(k):
    from monogs_amd.frames import Intrinsics
    return Intrinsics(k, DEV)


def _mesh(v, t, colors=None):
    from monogs_amd.tsdf import TriangleMesh
    return TriangleMesh(_dev(v), _dev(np.asarray(t, np.int32)), None if colors is None else _dev(colors))


_renderers = {}


def _renderer(k):
    from monogs_amd.mesh_render import MeshRenderer
    key = (k["W"], k["H"], k["fx"], k["cx"])
    if key not in _renderers:
        _renderers[key] = MeshRenderer(_intr(k), DEV)
    return _renderers[key]


def _labels(T):
    return ((np.arange(T, dtype=np.int64) * 7 + 3) % 11).astype(np.int32)


def _render_case(c, want=("depth", "tri_id", "rgb", "label"), bg=(0.25, 0.5, 0.75)):
    """The case on the device: numpy copies of the wanted images, and the status word."""
    r = _renderer(c["intr"])
    lab = _labels(len(c["triangles"]))
    out = r.render(_mesh(c["vertices"], c["triangles"], c["colors"]), _dev(c["R"]), _dev(c["t"]), want=want, face_labels=_dev(lab), bg=bg,
                   near=c["near"], far=c["far"], two_sided=c["two_sided"])
    got = {k: v.cpu().numpy().copy() for k, v in out.items()}
    got["status"] = int(r.status_word().cpu().item())
    r.status_word().zero_()
    return got, lab


def _mirror(c):
    return M.render(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], colors=c["colors"], near=c["near"], far=c["far"],
                    two_sided=c["two_sided"])


def _check_against_mirror(c, got, lab, m, bg=(0.25, 0.5, 0.75)):
    """The tolerances of the header; returns the share of ambiguous pixels."""
    una = ~m["ambiguous"]
    depth, ids = got["depth"].astype(np.float64), got["tri_id"]
    hit = depth > 0
    assert (hit == m["hit"])[una].all(), int((hit != m["hit"])[una].sum())
    both = una & hit
    err = np.abs(depth - m["depth"])[both] / m["depth"][both] if both.any() else np.zeros(1)
    print(f"  {int(hit.sum())} hit, {int(m['ambiguous'].sum())} ambiguous, worst relative depth error {err.max():.3e}", end="")
    assert err.max() <= MC.DEPTH_RTOL, err.max()
    assert ((ids >= 0) == hit).all() and (ids[~hit] == -1).all()
    ok, z = M.grown_accepts(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], ids, c["near"], c["far"], c["two_sided"])
    assert ok[both].all(), int((~ok)[both].sum())
    assert (np.abs(z - depth)[both] <= MC.DEPTH_RTOL * depth[both]).all()
    if "label" in got:
        assert (got["label"][hit] == lab[ids[hit]]).all() and (got["label"][~hit] == -1).all()
    if "rgb" in got and m["rgb"] is not None:
        same = both & (ids == m["tri_id"])                       # (another triangle at an edge: another interpolation of the same colours)
        cerr = np.abs(got["rgb"].astype(np.float64) - m["rgb"])[:, same]
        print(f", worst colour error {cerr.max() if cerr.size else 0.0:.3e}", end="")
        assert cerr.size == 0 or cerr.max() <= MC.COLOR_ATOL, cerr.max()
        assert (got["rgb"][:, ~hit] == np.array(bg, np.float32)[:, None]).all()
    print()
    return float(m["ambiguous"].mean())


@pytest.mark.parametrize("name", [n for n in MC.small_cases()])
def test_small_cases_against_the_mirror(native_lib, name):
    c = MC.small_cases()[name]
    got, lab = _render_case(c)
    m = _mirror(c)
    print(name, end=":")
    share = _check_against_mirror(c, got, lab, m)
    assert share <= MC.AMBIGUOUS_CAP and got["status"] == 0
    owners = set(got["tri_id"].reshape(-1).tolist()) - {-1}
    if c["hits"] is not None:
        assert owners == c["hits"], owners
    if name == "reversed_one_sided":
        assert len(owners) == 1, owners                      # two_sided=False drops exactly one of the two
    if name == "wholly_behind":
        assert not got["depth"].any()
    if name == "fine_plane":
        assert len(owners) < 0.1 * len(c["triangles"])       # most triangles cover no pixel centre
        assert (got["depth"] == 0).any() and (got["depth"] > 0).sum() > 2000


def test_the_same_triangle_twice_names_the_smaller_index(native_lib):
    c = MC.small_cases()["same_triangle_twice"]
    got, _ = _render_case(c)
    assert (got["depth"] > 0).sum() > 100 and (got["tri_id"][got["depth"] > 0] == 0).all()


def _sphere_mesh():
    from monogs_amd.tsdf import TSDFVolume
    c = TC.sphere_case()
    vol = TSDFVolume(c["origin"], c["s"], c["dims"], DEV, color=False)
    p = vol.planes()
    p[0].copy_(_dev(c["tsdf"]))
    p[1].copy_(_dev(c["weight"]))
    return vol.extract(c["min_weight"]), c["centre"]


@pytest.mark.parametrize("which", ["octahedron", "tsdf_sphere"])
def test_watertight_exactly(native_lib, which):
    """A camera inside a closed surface whose triangles share their vertices by index: not one pixel without a hit."""
    if which == "octahedron":
        v, t = MC.octahedron()
        mesh, centre = _mesh(v, t), (0.0, 0.0, 0.0)
    else:
        mesh, centre = _sphere_mesh()
        assert mesh.triangles.shape[0] > 1000
    r = _renderer(MC.INTR_48)
    for R, t in MC.inside_poses(centre):
        out = r.render(mesh, _dev(R), _dev(t), want=("depth", "tri_id"))
        depth = out["depth"].cpu().numpy()
        assert (depth > 0).all(), int((depth <= 0).sum())
        assert (out["tri_id"].cpu().numpy() >= 0).all()
    assert r.status() == 0


@pytest.mark.parametrize("bad", ["V", "-1"])
def test_out_of_range_index(native_lib, bad):
    v, t = MC.octahedron()
    R, tt = MC.inside_poses()[1]
    r = _renderer(MC.INTR_48)
    before = {k: x.cpu().numpy().copy() for k, x in r.render(_mesh(v, t), _dev(R), _dev(tt), want=("depth", "tri_id")).items()}
    assert r.status() == 0
    k = int(before["tri_id"][20, 20])
    t2 = t.copy()
    t2[k, 1] = len(v) if bad == "V" else -1
    after = {k_: x.cpu().numpy().copy() for k_, x in r.render(_mesh(v, t2), _dev(R), _dev(tt), want=("depth", "tri_id")).items()}
    assert int(r.status_word().cpu().item()) & 1
    with pytest.raises(Exception, match="outside"):
        r.status()
    assert r.status() == 0                                   # raising cleared it
    assert not (after["tri_id"] == k).any()
    keep = before["tri_id"] != k
    assert keep.sum() > 1000 and (~keep).sum() >= 1
    assert np.array_equal(after["depth"][keep], before["depth"][keep]) and np.array_equal(after["tri_id"][keep], before["tri_id"][keep])
    # the octahedron has one layer: a hole where the triangle was (but for a pixel centre exactly on an edge, which the neighbour owns too)
    assert (after["depth"][~keep] == 0).sum() >= 0.9 * (~keep).sum()


@pytest.fixture(scope="module")
def room():
    """The coloured room mesh at max_edge 0.25 with its surface ids, pose 3 of the six, the mirror's render and the ray cast's."""
    from monogs_amd.sequences import raycast_room, room_mesh, room_mesh_surface_ids
    mesh = room_mesh(DEV, MC.ROOM_MAX_EDGE, colors=True)
    sid = room_mesh_surface_ids(MC.ROOM_MAX_EDGE)
    poses = MC.room_poses()
    R, t = poses[MC.ROOM_POSE]
    c = dict(vertices=mesh.vertices.cpu().numpy(), triangles=mesh.triangles.cpu().numpy(), colors=mesh.colors.cpu().numpy(), R=R, t=t,
             intr=MC.ROOM_INTR, near=0.01, far=0.0, two_sided=True)
    m = _mirror(c)
    rgb, depth, ids = raycast_room(torch.from_numpy(R), torch.from_numpy(t), MC.ROOM_INTR, DEV, with_ids=True)
    return dict(mesh=mesh, sid=sid, poses=poses, case=c, mirror=m, ray=(rgb.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()))


def test_room_against_the_mirror_and_the_ray_cast(native_lib, room):
    c, m = room["case"], room["mirror"]
    r = _renderer(MC.ROOM_INTR)
    sid = room["sid"].numpy()
    out = r.render(room["mesh"], _dev(c["R"]), _dev(c["t"]), want=("depth", "tri_id", "rgb", "label"), face_labels=room["sid"].to(DEV),
                   bg=(0.25, 0.5, 0.75))
    got = {k: v.cpu().numpy().copy() for k, v in out.items()}
    assert r.status() == 0
    print("room", end=":")
    share = _check_against_mirror(c, got, sid, m)
    assert share <= MC.AMBIGUOUS_CAP
    una = ~m["ambiguous"]
    assert (got["depth"] > 0)[una].all()                     # (duplicated vertices along the creases: holes only at ambiguous pixels)
    _, rd, rid = room["ray"]
    err = np.abs(got["depth"].astype(np.float64) - rd)[una]
    print(f"room against raycast_room: worst depth difference {err.max():.3e} m")
    assert (err <= MC.DEPTH_RTOL * rd[una] + MC.RAYCAST_ATOL).all(), err.max()
    assert (got["label"][una] == rid[una]).all()


def test_order_and_reproducibility(native_lib, room):
    c, m = room["case"], room["mirror"]
    r = _renderer(MC.ROOM_INTR)
    R, t = _dev(c["R"]), _dev(c["t"])
    a = {k: v.clone() for k, v in r.render(room["mesh"], R, t, want=("depth", "tri_id", "rgb")).items()}
    b = r.render(room["mesh"], R, t, want=("depth", "tri_id", "rgb"))
    assert all(torch.equal(a[k], b[k]) for k in a)
    perm = np.random.default_rng(5).permutation(len(c["triangles"]))          # new triangle n is old triangle perm[n]
    shuffled = _mesh(c["vertices"], c["triangles"][perm], c["colors"])
    s = r.render(shuffled, R, t, want=("depth", "tri_id"))
    assert torch.equal(s["depth"], a["depth"])
    ids_a, ids_s = a["tri_id"].cpu().numpy(), s["tri_id"].cpu().numpy()
    u = m["unique"] & (ids_a >= 0)
    assert u.sum() > 0.9 * u.size and (perm[ids_s[u]] == ids_a[u]).all()
    assert r.status() == 0


def test_small_triangles_finished_by_the_setup_kernel_change_nothing(native_lib, room):
    """Triangles whose padded box is at most 4 x 4 pixels never reach the raster pass; with the test flag they do: the same bits."""
    want = ("depth", "tri_id", "rgb")
    c = MC.small_cases()["fine_plane"]
    mesh, R, t = _mesh(c["vertices"], c["triangles"], c["colors"]), _dev(c["R"]), _dev(c["t"])
    r = _renderer(c["intr"])
    a = {k: v.clone() for k, v in r.render(mesh, R, t, want=want).items()}
    b = r.render(mesh, R, t, want=want, fuse_small=False)
    assert all(torch.equal(a[k], b[k]) for k in want) and int((a["depth"] > 0).sum()) > 2000
    from monogs_amd.sequences import room_mesh
    fine = room_mesh(DEV, 0.05, colors=True)                  # a mix: small triangles far away, larger ones near the camera
    R, t = _dev(room["case"]["R"]), _dev(room["case"]["t"])
    r = _renderer(MC.ROOM_INTR)
    a = {k: v.clone() for k, v in r.render(fine, R, t, want=want).items()}
    b = r.render(fine, R, t, want=want, fuse_small=False)
    assert all(torch.equal(a[k], b[k]) for k in want) and bool((a["depth"] > 0).all())
    assert r.status() == 0


def test_capture(native_lib, room):
    """One stream, no parallel branches: the graph replayed after the pose tensors were rewritten in place is the eager render."""
    from monogs_amd.mesh_render import MeshRenderer
    r = MeshRenderer(_intr(MC.ROOM_INTR), DEV)
    poses = room["poses"]
    R, t = _dev(poses[0][0]).clone(), _dev(poses[0][1]).clone()
    want = ("depth", "tri_id", "rgb")
    r.render(room["mesh"], R, t, want=want)                   # (scratch and outputs exist before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = r.render(room["mesh"], R, t, want=want)
    R.copy_(_dev(poses[4][0]))
    t.copy_(_dev(poses[4][1]))
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in out.items()}
    eager = MeshRenderer(_intr(MC.ROOM_INTR), DEV).render(room["mesh"], _dev(poses[4][0]), _dev(poses[4][1]), want=want)
    assert all(torch.equal(replayed[k], eager[k]) for k in want)
    first = MeshRenderer(_intr(MC.ROOM_INTR), DEV).render(room["mesh"], _dev(poses[0][0]), _dev(poses[0][1]), want=want)
    assert not torch.equal(first["depth"], eager["depth"])
    del graph


def test_depth_l1_kernel(native_lib):
    from monogs_amd.mesh_render import depth_l1_row
    a, b = MC.depth_l1_images()
    for md in (0.0, MC.DEPTH_L1_MAX):
        want = M.depth_l1(a, b, md)
        row = depth_l1_row(_dev(a), _dev(b), md)
        again = depth_l1_row(_dev(a), _dev(b), md)
        got = row.cpu().tolist()
        print(f"depth_l1 max_depth {md}: {got} against {want}")
        assert abs(got[0] - want[0]) <= 1e-12 * want[0] and got[1] == want[1] and got[2] == want[2]
        assert torch.equal(row, again)
        assert 0 < want[1] < want[2] < a.size
    big = np.abs(np.random.default_rng(2).normal(2.0, 0.5, (300, 700))).astype(np.float32)       # more than one workgroup
    want = M.depth_l1(big, big[::-1].copy(), 0.0)
    got = depth_l1_row(_dev(big), _dev(big[::-1].copy())).cpu().tolist()
    assert abs(got[0] - want[0]) <= 1e-12 * want[0] and got[1:] == [want[1], want[2]]


def test_eval_depth_l1_of_the_displaced_room(native_lib, room):
    from monogs_amd.mesh_render import eval_depth_l1
    from monogs_amd.tsdf import TriangleMesh
    gt = room["mesh"]
    rec = TriangleMesh(gt.vertices + torch.tensor([0.0, 0.0, 0.02], device=DEV), gt.triangles, None)      # 2 cm along the z walls' normal
    views = [(_dev(R), _dev(t)) for R, t in room["poses"][:3]]
    out = eval_depth_l1(rec, gt, views, _intr(MC.ROOM_INTR))
    assert out["readbacks"] == 1 and out["views"] == 3 and len(out["per_view"]) == 3
    c = room["case"]
    rv = rec.vertices.cpu().numpy()
    means, both, in_gt = [], 0, 0
    for R, t in room["poses"][:3]:
        ma = M.render(rv, c["triangles"], R, t, MC.ROOM_INTR)
        mb = M.render(c["vertices"], c["triangles"], R, t, MC.ROOM_INTR)
        s, n, g = M.depth_l1(ma["depth"], mb["depth"])
        means.append(s / n)
        both, in_gt = both + n, in_gt + g
    want, cov = sum(means) / 3, both / in_gt
    print(f"eval_depth_l1: {out['depth_l1_m']:.6f} m against {want:.6f} m, coverage {out['coverage']:.6f} against {cov:.6f}")
    # (a handful of ambiguous pixels per view may flip between surfaces metres apart: their share of the mean, on top of the tolerance)
    slack = 3 * MC.AMBIGUOUS_CAP
    assert abs(out["depth_l1_m"] - want) <= MC.DEPTH_RTOL * 6.0 + slack * want + 1e-9, (out["depth_l1_m"], want)
    assert abs(out["coverage"] - cov) <= MC.AMBIGUOUS_CAP and 0.005 < want < 0.05


def test_eval_reconstruction_with_rendered_depths(native_lib, room):
    from monogs_amd import mesh_eval as ME
    from monogs_amd.mesh_render import MeshRenderer
    from monogs_amd.sequences import room_mesh
    from monogs_amd.tsdf import TriangleMesh
    gt = room_mesh(DEV, 0.1)
    rec = TriangleMesh(gt.vertices + torch.tensor([0.004, -0.003, 0.005], device=DEV), gt.triangles, None)
    intr = _intr(MC.ROOM_INTR)
    views = [(_dev(R), _dev(t)) for R, t in room["poses"][:3]]
    r = MeshRenderer(intr, DEV)
    depths = [r.render(gt, R, t)["depth"].clone() for R, t in views]
    a = ME.eval_reconstruction(rec, gt, n_samples=20_000, viewpoints=views, intr=intr, depths="render")
    b = ME.eval_reconstruction(rec, gt, n_samples=20_000, viewpoints=views, intr=intr, depths=depths)
    assert a == b and a["readbacks"] == 1
    plain = ME.eval_reconstruction(rec, gt, n_samples=20_000, viewpoints=views, intr=intr)
    assert a["gt_area_m2"] < plain["gt_area_m2"]              # the occlusion test removes what the boxes hide
    seen = ME.seen_vertices(rec, views, intr, depths="render", occluder=gt)
    assert torch.equal(seen, ME.seen_vertices(rec, views, intr, depths=depths))
    with pytest.raises(ValueError, match="occluder"):
        ME.seen_vertices(rec, views, intr, depths="render")


@pytest.fixture(scope="module")
def mesh_sequence():
    from monogs_amd.sequences import make_mesh_sequence, room_mesh, room_mesh_surface_ids
    mesh = room_mesh(DEV, MC.SEQ_MAX_EDGE, colors=True)
    sid = room_mesh_surface_ids(MC.SEQ_MAX_EDGE).to(DEV)
    poses = MC.room_poses()[:4]
    frames, intr = make_mesh_sequence(mesh, poses, MC.INTR_48_ROOM, DEV, face_labels=sid)
    return mesh, sid, poses, frames, intr


def test_make_mesh_sequence(native_lib, mesh_sequence):
    from monogs_amd.mesh_render import MeshRenderer
    from monogs_amd.sequences import raycast_room
    mesh, sid, poses, frames, intr = mesh_sequence
    assert len(frames) == 4 and (intr.width, intr.height) == (48, 36)
    r = MeshRenderer(intr, DEV)
    v, t = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    for f, (R, tt) in zip(frames, poses):
        out = r.render(mesh, _dev(R), _dev(tt), want=("depth", "rgb", "label"), face_labels=sid)
        assert torch.equal(f.depth, out["depth"]) and torch.equal(f.rgb, out["rgb"]) and torch.equal(f.segmentation, out["label"])
        assert torch.equal(f.R_gt.cpu(), torch.from_numpy(R)) and torch.equal(f.T_gt.cpu(), torch.from_numpy(tt))
        m = M.render(v, t, R, tt, MC.INTR_48_ROOM)
        una = ~m["ambiguous"]
        assert m["ambiguous"].mean() <= MC.AMBIGUOUS_CAP
        rgb = raycast_room(torch.from_numpy(R), torch.from_numpy(tt), MC.INTR_48_ROOM, DEV)[0]
        d = (f.rgb - rgb).abs().cpu().numpy()
        print(f"make_mesh_sequence frame {f.frame_idx}: colour against raycast_room mean {d.mean():.4f}, worst {d[:, una].max():.4f}")
        assert d[:, una].max() <= 0.1
    with pytest.raises(ValueError, match="colours"):
        from monogs_amd.sequences import make_mesh_sequence, room_mesh
        make_mesh_sequence(room_mesh(DEV, 0.5), poses, MC.INTR_48_ROOM, DEV)


def test_run_slam_with_depth_l1(native_lib, tmp_path):
    from monogs_amd.sequences import make_mesh_sequence, room_mesh
    from monogs_amd.slam_harness import run_slam
    mesh = room_mesh(DEV, 0.05, colors=True)
    seq = make_mesh_sequence(mesh, MC.slam_poses(4), TC.ROOM_INTR, DEV)
    run = dict(n_frames=4, intrinsics=TC.ROOM_INTR, tracking_itr_num=40, mapping_itr_num=30, init_itr_num=300, window_size=4,
               kf_interval=2, scene="room", mesh_voxel=0.04)
    today = {"path", "vertices", "triangles", "voxel", "integrate_ms", "extract_ms"}
    out = run_slam(sequence=seq, mesh_path=str(tmp_path / "a.ply"), mesh_gt="room", mesh_samples=20_000, mesh_depth_l1=True, **run)
    assert set(out["mesh"]) == today | {"reconstruction", "depth_l1"}, set(out["mesh"])
    d = out["mesh"]["depth_l1"]
    print(f"run_slam depth_l1: {d}")
    assert d["readbacks"] == 1 and d["views"] >= 2 and math.isfinite(d["depth_l1_m"]) and 0 < d["coverage"] <= 1
    assert all(math.isfinite(float(x)) for x in out["mesh"]["reconstruction"].values())
    assert all(math.isfinite(p["depth_l1_m"]) for p in d["per_view"])
    seq = make_mesh_sequence(mesh, MC.slam_poses(4), TC.ROOM_INTR, DEV)
    plain = run_slam(sequence=seq, mesh_path=str(tmp_path / "b.ply"), mesh_gt="room", mesh_samples=20_000, **run)
    assert set(plain["mesh"]) == today | {"reconstruction"} and set(plain) == set(out)
