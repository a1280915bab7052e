"""TEST INFRASTRUCTURE: the inputs tests/test_gpu_mesh_render.py feeds the mesh renderer, as float32 numpy arrays, so that
tests/test_mesh_render_host.py can run tests/mesh_render_mirror.py over the very same inputs without a GPU (the share of ambiguous
pixels, the error of the float32 restatement).  Vertices, principal points and poses are off every lattice: a pixel centre that lies
exactly on a triangle's edge is ambiguous.

The tolerances of the GPU test are 4 x the largest error of the mirror's float32 restatement against float64 over these cases and
the room (the margin: the kernel's operation order and contraction differ from numpy's):

    depth   F32_DEPTH_REL = 3.5e-6 relative  (measured: 3.41e-6 on the room's six poses, 7.4e-7 on the small cases)
    colour  F32_COLOR_ABS = 1.5e-5 absolute  (measured: 1.39e-5 on the room, 1.45e-5 on the fine plane)

tests/test_mesh_render_host.py measures both again, prints them and asserts they stay within these figures."""
import numpy as np

import tsdf_cases as TC

AMBIGUOUS_CAP = TC.AMBIGUOUS_CAP                  # 2e-3: the TSDF test's
F32_DEPTH_REL, F32_COLOR_ABS = 3.5e-6, 1.5e-5
DEPTH_RTOL, COLOR_ATOL = 4 * F32_DEPTH_REL, 4 * F32_COLOR_ABS
RAYCAST_ATOL = 1e-5                               # raycast_room's own float32 error: 1.3e-6 m measured (host test), margin 8

INTR_37 = dict(fx=33.1, fy=32.7, cx=18.3, cy=14.6, W=37, H=29)
INTR_48 = dict(fx=TC.FX, fy=TC.FY, cx=TC.CX, cy=TC.CY, W=TC.W, H=TC.H)
INTR_48_ROOM = dict(fx=40.1, fy=40.5, cx=23.7, cy=18.3, W=48, H=36)          # the room, wide
INTR_64 = dict(fx=55.3, fy=54.1, cx=31.7, cy=24.3, W=64, H=48)
ROOM_INTR, ROOM_MAX_EDGE, ROOM_POSE = TC.ROOM_INTR, 0.25, 3
SEQ_MAX_EDGE = 0.04        # make_mesh_sequence: the texture, sampled at the vertices of 4 cm edges, is within 0.075 of itself on every edge


def pose(k=0):
    return TC.poses()[k]


def _colors(v):
    return np.stack([0.5 + 0.45 * np.sin(3.0 * v[:, 0] + 0.3), 0.5 + 0.45 * np.cos(2.0 * v[:, 1]), 0.5 + 0.4 * np.sin(v[:, 2] + v[:, 0])], 1).astype(np.float32)


def _case(vertices, triangles, intr=INTR_48, k=0, **kw):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    R, t = pose(k)
    return dict(dict(vertices=v, triangles=np.asarray(triangles, np.int32).reshape(-1, 3), colors=_colors(v), R=R, t=t, intr=intr, near=0.01,
                     far=0.0, two_sided=True), **kw)


FRONT = [(-0.513, -0.402, 2.107), (0.611, -0.317, 2.303), (0.047, 0.553, 1.911)]
SECOND = [(-0.893, 0.207, 2.611), (-0.107, 0.813, 2.489), (-0.951, 0.857, 2.703)]


def small_cases():
    """name -> case.  ``hits``: the triangles that must own at least one pixel; every other triangle must own none."""
    c = {}
    c["facing"] = _case(FRONT, [(0, 1, 2)], hits={0})
    det = lambda p: float(np.linalg.det(np.array(p, np.float64)))  # noqa: E731
    second = (3, 5, 4) if det(FRONT) * det(SECOND) > 0 else (3, 4, 5)            # wound against the first, as seen from near the origin
    c["reversed_two_sided"] = _case(FRONT + SECOND, [(0, 1, 2), second], hits={0, 1})
    c["reversed_one_sided"] = _case(FRONT + SECOND, [(0, 1, 2), second], two_sided=False, hits=None)        # exactly one of the two
    c["one_vertex_behind"] = _case([(-0.413, -0.302, 1.507), (0.511, -0.217, 1.203), (0.107, 0.403, -0.811)], [(0, 1, 2)], hits={0})
    c["wholly_behind"] = _case([(-0.513, -0.402, -2.107), (0.611, -0.317, -2.303), (0.047, 0.553, -1.911)], [(0, 1, 2)], hits=set())
    far = [(x * 2.5, y * 2.5, z * 2.5) for x, y, z in FRONT]
    c["beyond_far"] = _case(FRONT + far, [(0, 1, 2), (3, 4, 5)], far=3.0, hits={0})
    close = [(x * 0.1, y * 0.1, z * 0.1) for x, y, z in FRONT]
    c["nearer_than_near"] = _case(FRONT + close, [(0, 1, 2), (3, 4, 5)], near=0.5, hits={0})
    # zero area: two vertices at one position under two indices; a repeated index; and an honest triangle behind both
    c["zero_area"] = _case(SECOND + [FRONT[0], FRONT[1], FRONT[1]], [(3, 4, 5), (3, 4, 4), (0, 1, 2)], hits={2})
    c["same_triangle_twice"] = _case(FRONT, [(0, 1, 2), (0, 1, 2)], hits={0})
    # two triangles over the whole 37 x 29 image (no multiple of 8: edge blocks), tilted
    quad = [(-3.013, -2.507, 2.211), (3.107, -2.411, 2.513), (3.011, 2.603, 2.809), (-3.109, 2.497, 2.407)]
    c["whole_image"] = _case(quad, [(0, 1, 2), (0, 2, 3)], intr=INTR_37, k=1, hits={0, 1})
    c["fine_plane"] = fine_plane()
    return c


def fine_plane(nx=200, ny=150, step=0.0108):
    """A tilted plane at about 2 m diced to about 0.3 pixels per edge at 64 x 48 (60 000 triangles): most cover no pixel centre.  It
    leaves a border of the image uncovered."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    x, y = (i - nx / 2) * step + 0.0137, (j - ny / 2) * step - 0.0071
    v = np.stack([x, y, 2.013 + 0.11 * x - 0.07 * y], -1).reshape(-1, 3)
    ci, cj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    v00 = (ci * (ny + 1) + cj).reshape(-1)
    v10, v01, v11 = v00 + ny + 1, v00 + 1, v00 + ny + 2
    tri = np.stack([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)], 1).reshape(-1, 3)
    return _case(v, tri, intr=INTR_64, hits=None)


def octahedron(levels=3, radius=1.5, seed=3):
    """A subdivided octahedron (8 x 4^levels = 512 triangles) on a sphere around the origin, with shared vertices, shuffled vertex
    numbering, shuffled triangle order and a third of the windings flipped: ``(vertices [V,3] f32, triangles [T,3] i32)``."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    verts = [np.array(v, np.float64) for v in verts]
    for _ in range(levels):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, cc in tris:
            ab, bc, ca = m(a, b), m(b, cc), m(cc, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, cc), (ab, bc, ca)]
        tris = out
    rng = np.random.default_rng(seed)
    v = np.stack(verts) * radius * (1.0 + 0.1 * np.sin(7.0 * np.stack(verts)[:, :1] + 1.3))      # a bumpy sphere: no two faces coplanar
    t = np.array(tris, np.int64)
    perm = rng.permutation(len(v))                 # new number of old vertex n: perm[n]
    v2 = np.empty_like(v)
    v2[perm] = v
    t = perm[t]
    t = t[rng.permutation(len(t))]
    flip = rng.random(len(t)) < 1 / 3
    t[flip] = t[flip][:, [0, 2, 1]]
    return v2.astype(np.float32), t.astype(np.int32)


def inside_poses(centre=(0.0, 0.0, 0.0)):
    """Three world->camera poses of a camera standing near ``centre``, turned three ways."""
    c = np.asarray(centre, np.float64)
    out = []
    for rx, ry, rz, off in ((0.013, -0.021, 0.007, (0.011, -0.017, 0.023)), (0.9, 2.1, -0.4, (-0.031, 0.027, 0.013)),
                            (-1.3, -0.7, 2.9, (0.023, 0.019, -0.029))):
        R = TC._rot(rx, ry, rz).astype(np.float64)
        out.append((R.astype(np.float32), (-(R @ (c + np.array(off)))).astype(np.float32)))
    return out


def room_poses(n=6, step_scale=40):
    """The world->camera poses of ``make_room_sequence(n, step_scale=step_scale)`` as ``(R, t)`` float32 numpy (through the sequence
    itself, on the CPU, at 4 x 4 pixels)."""
    from monogs_amd.sequences import make_room_sequence
    frames, _ = make_room_sequence(n, dict(fx=4.0, fy=4.0, cx=2.0, cy=2.0, W=4, H=4), device="cpu", step_scale=step_scale)
    return [(f.R_gt.numpy().astype(np.float32), f.T_gt.numpy().astype(np.float32)) for f in frames]


def slam_poses(n):
    """The poses ``run_slam(scene="room")`` would generate for ``n`` frames."""
    return room_poses(n, 1.0)


def depth_l1_images(W=37, H=29):
    """Two depth images with zeros (holes) in different places; MAX_DEPTH cuts some pixels of each."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a = 1.5 + 0.031 * (x - 18) + 0.023 * (y - 14) + 0.05 * np.sin(0.7 * x)
    b = a + 0.02 * np.cos(0.4 * y) - 0.013
    a[3:7, 5:11] = 0.0
    b[5:9, 8:15] = 0.0
    b[20:, 30:] = 0.0
    return a.astype(np.float32), b.astype(np.float32)


DEPTH_L1_MAX = 1.9
