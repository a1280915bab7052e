"""Mesh rendering without a GPU: the float64 mirror of the specification (tests/mesh_render_mirror.py) against the closed form of
``raycast_room``, the share of ambiguous pixels of every case the GPU test uses, the error of the mirror's float32 restatement (what
the GPU tolerances are 4 x of), ``room_mesh_surface_ids``, the ABI with its argument refusals, the host API and the pose-file parser.

Measured here (printed by the tests): mirror against ``raycast_room`` at 160 x 120 over the six room poses 1.3e-6 m at worst and no
hole; at most 15 of 19 200 pixels ambiguous (7.8e-4); float32 restatement 3.41e-6 relative in depth and 1.39e-5 in colour on the room,
7.4e-7 and 1.45e-5 on the small cases."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mesh_render_cases as MC
import mesh_render_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mgs_mesh_render_scratch_bytes", "mgs_mesh_render", "mgs_depth_l1_scratch_bytes", "mgs_depth_l1")


def _f32_error(c, a):
    """(largest relative depth error, largest absolute colour error, hit / no-hit differences) of the float32 restatement against
    the float64 render ``a``, at the pixels neither calls ambiguous."""
    b = M.render(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], colors=c["colors"], near=c["near"], far=c["far"],
                 two_sided=c["two_sided"], dtype=np.float32)
    una = ~a["ambiguous"] & ~b["ambiguous"]
    both = una & a["hit"] & b["hit"]
    if not both.any():
        return 0.0, 0.0, int((a["hit"] != b["hit"])[una].sum())
    same = both & (a["tri_id"] == b["tri_id"])
    return (float((np.abs(b["depth"] - a["depth"])[both] / a["depth"][both]).max()), float(np.abs(b["rgb"] - a["rgb"])[:, same].max()),
            int((a["hit"] != b["hit"])[una].sum()))


@pytest.fixture(scope="module")
def room_renders():
    """The mirror's render of the coloured room (max_edge 0.25) from the six poses, with the ray cast's images."""
    from monogs_amd.sequences import raycast_room, room_mesh, room_mesh_surface_ids
    mesh = room_mesh("cpu", MC.ROOM_MAX_EDGE, colors=True)
    sid = room_mesh_surface_ids(MC.ROOM_MAX_EDGE).numpy()
    assert sid.shape == (mesh.triangles.shape[0],) and mesh.colors.shape == mesh.vertices.shape
    out = []
    for R, t in MC.room_poses():
        c = dict(vertices=mesh.vertices.numpy(), triangles=mesh.triangles.numpy(), colors=mesh.colors.numpy(), R=R, t=t, intr=MC.ROOM_INTR,
                 near=0.01, far=0.0, two_sided=True)
        m = M.render(c["vertices"], c["triangles"], R, t, MC.ROOM_INTR, colors=c["colors"])
        rgb, depth, ids = raycast_room(torch.from_numpy(R), torch.from_numpy(t), MC.ROOM_INTR, "cpu", with_ids=True)
        out.append((c, m, depth.numpy().astype(np.float64), ids.numpy()))
    return sid, out


def test_mirror_against_the_closed_form(room_renders):
    _, renders = room_renders
    worst = 0.0
    for c, m, depth, _ in renders:
        assert m["hit"].all()                                  # no holes
        worst = max(worst, float(np.abs(m["depth"] - depth).max()))
    print(f"mirror against raycast_room: worst difference {worst:.3e} m over {len(renders)} poses")
    assert worst <= 2e-6                                       # raycast_room is float32 at up to 7 m: 1.3e-6 m measured


def test_ambiguous_share_of_every_gpu_case(room_renders):
    _, renders = room_renders
    for n, (c, m, _, _) in enumerate(renders):
        print(f"room pose {n}: {int(m['ambiguous'].sum())} of {m['ambiguous'].size} pixels ambiguous")
        assert m["ambiguous"].mean() <= MC.AMBIGUOUS_CAP
    for name, c in MC.small_cases().items():
        m = M.render(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], near=c["near"], far=c["far"], two_sided=c["two_sided"])
        print(f"{name}: {int(m['hit'].sum())} hit, {int(m['ambiguous'].sum())} ambiguous")
        assert m["ambiguous"].mean() <= MC.AMBIGUOUS_CAP, name
        owners = set(m["tri_id"].reshape(-1).tolist()) - {-1}
        if c["hits"] is not None:
            assert owners == c["hits"], (name, owners)
    one = M.render(**{k: v for k, v in MC.small_cases()["reversed_one_sided"].items() if k not in ("hits", "colors")})
    two = M.render(**{k: v for k, v in MC.small_cases()["reversed_two_sided"].items() if k not in ("hits", "colors")})
    assert len(set(one["tri_id"].reshape(-1).tolist()) - {-1}) == 1 and len(set(two["tri_id"].reshape(-1).tolist()) - {-1}) == 2
    twice = M.render(**{k: v for k, v in MC.small_cases()["same_triangle_twice"].items() if k not in ("hits", "colors")})
    assert not twice["unique"].any() and (twice["tri_id"][twice["hit"]] == 0).all()
    v, t = MC.octahedron()
    assert t.shape == (512, 3)
    for R, tt in MC.inside_poses():
        assert M.render(v, t, R, tt, MC.INTR_48)["hit"].all()


def test_float32_restatement(room_renders):
    _, renders = room_renders
    room_d = room_c = small_d = small_c = 0.0
    for c, m, _, _ in renders[::2] + renders[3:4]:
        d, col, flips = _f32_error(c, m)
        room_d, room_c = max(room_d, d), max(room_c, col)
        assert flips == 0
    for name, c in MC.small_cases().items():
        a = M.render(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], colors=c["colors"], near=c["near"], far=c["far"],
                     two_sided=c["two_sided"])
        d, col, flips = _f32_error(c, a)
        small_d, small_c = max(small_d, d), max(small_c, col)
        assert flips == 0, name
    print(f"float32 restatement: room depth {room_d:.3e} relative, colour {room_c:.3e}; small cases depth {small_d:.3e}, colour {small_c:.3e}")
    assert max(room_d, small_d) <= MC.F32_DEPTH_REL and max(room_c, small_c) <= MC.F32_COLOR_ABS
    assert MC.DEPTH_RTOL == 4 * MC.F32_DEPTH_REL and MC.COLOR_ATOL == 4 * MC.F32_COLOR_ABS


def test_the_culled_mirror_is_the_brute_force_one():
    for name in ("one_vertex_behind", "whole_image", "zero_area"):
        c = MC.small_cases()[name]
        kw = dict(colors=c["colors"], near=c["near"], far=c["far"], two_sided=c["two_sided"])
        a = M.render(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], **kw)
        b = M.render(c["vertices"], c["triangles"], c["R"], c["t"], c["intr"], tile=None, **kw)
        assert all(np.array_equal(a[k], b[k]) for k in ("depth", "tri_id", "rgb", "hit", "ambiguous", "unique")), name


def test_room_mesh_surface_ids(room_renders):
    sid, renders = room_renders
    for c, m, _, ids in renders:
        una = ~m["ambiguous"]
        assert (sid[m["tri_id"]][una] == ids[una]).all()
    from monogs_amd.sequences import ROOM_SURFACES, room_mesh, room_mesh_surface_ids
    assert set(sid.tolist()) == set(range(ROOM_SURFACES))
    for e in (0.1, 0.5):
        assert room_mesh_surface_ids(e).shape[0] == room_mesh("cpu", e).triangles.shape[0]
    plain, col = room_mesh("cpu", 0.5), room_mesh("cpu", 0.5, colors=True)
    assert plain.colors is None and torch.equal(plain.vertices, col.vertices) and torch.equal(plain.triangles, col.triangles)
    assert col.colors.dtype == torch.float32 and 0.02 <= float(col.colors.min()) and float(col.colors.max()) <= 0.98


def test_abi_version_and_symbols(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 25
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(native_lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        args = [a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[name][1]), (name, args)
    assert re.search(r"#define MGS_MESH_ONE_SIDED 1\b", text) and re.search(r"#define MGS_MESH_RENDER_MAX_IMAGE 16384\b", text)
    # the struct of the binding is the header's: 2 ints, 5 pointers, 2 ints, 6 floats, an int, 3 floats, 5 pointers
    assert C.sizeof(_lib.MgsMeshRender) == 8 + 5 * 8 + 8 + 6 * 4 + 4 + 3 * 4 + 5 * 8
    # a unit of its own: in the Makefile's SRCS, and included by nothing
    csrc = os.path.join(ROOT, "monogs_amd", "csrc")
    assert os.path.isfile(os.path.join(csrc, "mesh_render.hip"))
    assert re.search(r"^SRCS\s*=.*\bmesh_render\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    units = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    assert not [f for f in units if re.search(r'#\s*include\s+"[^"]*mesh_render\.\w+"', open(os.path.join(csrc, f)).read())]
    from monogs_amd import mesh_render
    assert re.search(r"#define MGS_MESH_NO_SMALL 2\b", text)
    assert (mesh_render.MESH_ONE_SIDED, mesh_render.MESH_NO_SMALL) == (1, 2)


def _params(**kw):
    from monogs_amd import _lib
    p = _lib.MgsMeshRender()
    q = 0x1000                             # non-NULL and never dereferenced: the refusals come before any launch
    p.V, p.T, p.W, p.H = 8, 4, 16, 16
    p.vertices, p.triangles, p.viewmatrix, p.depth, p.status = q, q, q, q, q
    p.fx, p.fy, p.cx, p.cy, p.near, p.far = 10.0, 10.0, 8.0, 8.0, 0.01, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bad_arguments_are_refused_before_any_launch(native_lib):
    L, q = native_lib, 0x1000
    err = lambda: L.mgs_last_error()  # noqa: E731
    call = lambda **kw: L.mgs_mesh_render(C.byref(_params(**kw)), q, None)  # noqa: E731
    assert L.mgs_mesh_render(None, q, None) == 1 and b"NULL" in err()
    assert call(V=-1) == 1 and b"negative" in err()
    assert call(T=-1) == 1 and b"negative" in err()
    assert call(T=(1 << 30) + 1) == 1 and b"2^30" in err()
    for kw in (dict(W=0), dict(H=0), dict(W=16385), dict(H=16385), dict(W=-3)):
        assert call(**kw) == 1 and b"image" in err(), kw
    assert call(fx=0.0) == 1 and b"fx and fy" in err()
    assert call(fy=-1.0) == 1 and b"fx and fy" in err()
    assert call(fx=float("nan")) == 1
    assert call(flags=4) == 1 and b"unknown flags" in err()
    for name in ("vertices", "triangles", "viewmatrix", "depth", "status"):
        assert call(**{name: None}) == 1 and b"non-NULL" in err(), name
    assert L.mgs_mesh_render(C.byref(_params()), None, None) == 1 and b"non-NULL" in err()
    assert call(rgb=q) == 1 and b"colors" in err()
    assert call(label=q) == 1 and b"face_labels" in err()
    f = L.mgs_depth_l1
    assert f(0, 16, q, q, 0.0, q, q, None) == 1 and b"image" in err()
    assert f(16, 16385, q, q, 0.0, q, q, None) == 1
    assert f(16, -1, q, q, 0.0, q, q, None) == 1
    for k in (2, 3, 5, 6):
        args = [16, 16, q, q, 0.0, q, q, None]
        args[k] = None
        assert f(*args) == 1 and b"non-NULL" in err(), k


def test_scratch_sizes_are_pure(native_lib):
    f = native_lib.mgs_mesh_render_scratch_bytes
    assert f(-1, 16, 16) == f(4, 0, 16) == f(4, 16, 16385) == f((1 << 30) + 1, 16, 16) == 256
    assert f(0, 16, 16) >= 16 * 16 * 8
    a, b, c = f(1000, 640, 480), f(100_000, 640, 480), f(1000, 1200, 680)
    assert a == f(1000, 640, 480) and b >= a + 99_000 * 64 and c >= a + (1200 * 680 - 640 * 480) * 8
    assert a >= 1000 * 64 + 2048 * 8 + 640 * 480 * 8
    assert native_lib.mgs_depth_l1_scratch_bytes() >= 1024 * 16


def test_host_api_refusals():
    from monogs_amd import mesh_eval, mesh_render, sequences
    from monogs_amd.frames import Intrinsics
    import monogs_amd
    assert monogs_amd.MeshRenderer is mesh_render.MeshRenderer and monogs_amd.eval_depth_l1 is mesh_render.eval_depth_l1
    intr = Intrinsics(MC.INTR_48, "cpu")
    mesh = sequences.room_mesh("cpu", 0.5)
    with pytest.raises(ValueError, match="colours"):
        sequences.make_mesh_sequence(mesh, MC.room_poses()[:1], MC.INTR_48, "cpu")
    with pytest.raises(ValueError, match="nonsense"):
        mesh_eval.eval_reconstruction(mesh, mesh, depths="nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        mesh_eval.eval_reconstruction(mesh, mesh, viewpoints=[], intr=intr, depths="nonsense")
    R, t = (torch.from_numpy(x) for x in MC.room_poses()[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_render.render_mesh(mesh, R, t, intr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_render.MeshRenderer(intr, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_render.depth_l1_row(torch.zeros(4, 4), torch.zeros(4, 4))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pose_file_parser():
    parse = _tool("mesh_eval").parse_poses
    text = "# two poses\n1 0 0 0.5  0 1 0 -0.25  0 0 1 2\n\n0,1,0,1, -1,0,0,2, 0,0,1,3   # commas too\n"
    poses = parse(text)
    assert poses == [([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [0.5, -0.25, 2.0]), ([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], [1.0, 2.0, 3.0])]
    assert parse("") == [] and parse("# nothing\n\n") == []
    with pytest.raises(ValueError, match="line 3"):
        parse("1 0 0 0 0 1 0 0 0 0 1 0\n\n1 2 3\n")
    with pytest.raises(ValueError, match="line 2"):
        parse("1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 x\n")
    with pytest.raises(ValueError, match="line 1"):
        parse("1 0 0 0 0 1 0 0 0 0 1 nan\n")
    with pytest.raises(ValueError, match="line 1"):
        parse("1 0 0 0 0 1 0 0 0 0 1 0 7\n")


def test_depth_l1_mirror():
    a, b = MC.depth_l1_images()
    s, n, g = M.depth_l1(a, b)
    s2, n2, g2 = M.depth_l1(a, b, MC.DEPTH_L1_MAX)
    assert 0 < n2 < n < g == g2 < a.size and 0 < s2 < s
