"""TEST INFRASTRUCTURE: the inputs tests/test_gpu_tsdf.py feeds the TSDF kernels, as float32 numpy arrays, so that
tests/test_tsdf_host.py can run tests/tsdf_mirror.py over the very same inputs without a GPU (the share of ambiguous voxels, the
room mesh against the room's closed-form surfaces)."""
import math

import numpy as np

import tsdf_mirror as M

# ---- integrate ----------------------------------------------------------------------------------------------------------------
# 37 x 20 x 19: x is no multiple of the 64-voxel brick and the total (14 060) is no multiple of a workgroup (256) or a scan block (2048).
# Origin, principal point and poses are off every lattice: a voxel centre that projects exactly onto a pixel boundary is ambiguous.
DIMS, S, TRUNC = (37, 20, 19), 0.05, 0.2
ORIGIN = (-0.913, -0.487, 1.013)
ORIGIN_CULLED = (0.487, 0.213, 1.613)          # most bricks outside the image or beyond depth_max + trunc
W, H = 48, 36
FX, FY, CX, CY = 41.3, 40.7, 23.7, 18.3
DEPTH_MIN, DEPTH_MAX, OPACITY_MIN, MAX_WEIGHT = 0.05, 1.62315, 0.9, 2.0      # (no pixel of depth_image lies within 4e-5 of DEPTH_MAX)
PX_MARGIN, M_MARGIN, AMBIGUOUS_CAP = 1e-4, 1e-5, 2e-3


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def poses():
    """Three world->camera poses.  The third stands inside the grid's depth range and is turned: part of the grid is behind the
    camera, part outside the image."""
    return [(_rot(0.013, -0.021, 0.007), np.array([0.011, -0.017, 0.023], np.float32)),
            (_rot(-0.05, 0.12, 0.03), np.array([-0.21, 0.04, 0.06], np.float32)),
            (_rot(0.08, -0.45, -0.02), np.array([0.33, -0.02, -1.27], np.float32))]


def depth_image(scale=1.0):
    """A tilted plane, a sphere in front of it, a zero-depth hole."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 1.5 + 0.0041 * (x - 24) + 0.0033 * (y - 18)
    r2 = ((x - 30.2) ** 2 + (y - 13.6) ** 2) / 64.0
    d = d - np.where(r2 < 1, 0.3 * np.sqrt(np.clip(1 - r2, 0, 1)), 0.0)
    d[5:9, 10:15] = 0.0
    return (d * scale).astype(np.float32)


def opacity_ramp():
    """0.8 .. 1.0 from left to right with a ripple: crosses OPACITY_MIN near the middle column."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return (0.8 + 0.2 * x / (W - 1) + 0.003 * np.sin(0.9 * y)).astype(np.float32)


def rgb_image():
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([0.5 + 0.4 * np.sin(0.21 * x + 0.1 * y), 0.5 + 0.4 * np.cos(0.17 * y), (x + y) / (W + H)]).astype(np.float32)


def frames(opacity: bool, color: bool):
    """The three frames of the integrate test.  With ``opacity`` the depth handed over is the un-normalised one (depth x opacity)."""
    out = []
    for n, (R, t) in enumerate(poses()):
        d = depth_image(0.36 if n == 2 else 1.0 + 0.01 * n)
        a = opacity_ramp() if opacity else None
        out.append(dict(depth=(d * a).astype(np.float32) if opacity else d, opacity=a, rgb=np.roll(rgb_image(), 3 * n, axis=2) if color else None,
                        R=R, t=t, depth_max=0.0 if n == 2 else DEPTH_MAX))
    return out


def run_mirror(frs, origin, color, dims=DIMS, s=S, trunc=TRUNC, max_weight=MAX_WEIGHT):
    """``(planes float64, visited-by-any [nz,ny,nx], ambiguous [nz,ny,nx], per-frame visited)`` of the mirror over ``frs``."""
    planes = M.new_planes(dims, color)
    amb = np.zeros(planes.shape[1:], dtype=bool)
    seen, per = np.zeros_like(amb), []
    for f in frs:
        live, mpx, mm = M.integrate(planes, origin, s, dims, f["depth"], f["R"], f["t"], FX, FY, CX, CY, trunc, DEPTH_MIN, f["depth_max"],
                                    f["opacity"], OPACITY_MIN, f["rgb"], max_weight)
        amb |= (mpx < PX_MARGIN) | (mm < M_MARGIN)
        seen |= live
        per.append(live)
    return planes, seen, amb, per


# ---- extract ------------------------------------------------------------------------------------------------------------------
def _colors(p):
    return np.stack([0.5 + 0.45 * np.sin(3.0 * p[..., 0]), 0.5 + 0.45 * np.cos(2.0 * p[..., 1]), 0.5 + 0.4 * np.sin(p[..., 2] + p[..., 0])]).astype(np.float32)


def sphere_case(n=32, s=0.05, r_vox=10.0, origin=(0.013, -0.021, 0.007), color=True):
    dims, r, trunc = (n, n, n), r_vox * s, 4 * s
    c = np.array(origin) + s * (n - 1) / 2 + np.array([0.011, 0.017, -0.013])          # off the lattice
    p = M.voxel_centres(origin, s, dims)
    t = np.clip((np.linalg.norm(p - c, axis=-1) - r) / trunc, -1, 1).astype(np.float32)
    return dict(dims=dims, s=s, origin=origin, tsdf=t, weight=np.ones_like(t), colors=_colors(p) if color else None, min_weight=1.0,
                centre=c, radius=r)


def extract_cases():
    """name -> dict(dims, s, origin, tsdf [nz,ny,nx] f32, weight, colors [3,nz,ny,nx] or None, min_weight)."""
    rng = np.random.default_rng(5)
    cases = {"sphere": sphere_case()}
    dims, s, origin = (9, 7, 5), 0.1, (-0.31, 0.12, 0.05)
    p = M.voxel_centres(origin, s, dims)
    n = np.array([0.48, 0.64, 0.6])
    t = np.clip((p @ n - 0.55) / 0.4, -1, 1).astype(np.float32)
    cases["plane"] = dict(dims=dims, s=s, origin=origin, tsdf=t, weight=np.ones_like(t), colors=None, min_weight=1.0)
    sp = sphere_case(n=16, r_vox=5.0)
    w = sp["weight"].copy()
    w[5:10, 3:9, 4:8] = 0.0                                                            # an unobserved block across the surface
    cases["unobserved_block"] = dict(sp, weight=w)
    sp = sphere_case(n=14, r_vox=4.5, color=False)
    cases["min_weight_2"] = dict(sp, weight=rng.integers(0, 4, size=sp["tsdf"].shape).astype(np.float32) + (rng.random(sp["tsdf"].shape) < 0.8) * 2.0,
                                 min_weight=2.0)
    i = np.arange(9, dtype=np.float32)[None, None, :] + np.zeros((5, 7, 1), np.float32)
    k = np.arange(5, dtype=np.float32)[:, None, None] + np.zeros((1, 7, 9), np.float32)
    t = np.clip((i - 4.0) / 4.0 + (k - 2.0) / 4.0, -1, 1).astype(np.float32)                        # exactly 0 wherever i + k = 6
    cases["exact_zero"] = dict(dims=dims, s=s, origin=origin, tsdf=t, weight=np.ones_like(t), colors=_colors(p), min_weight=1.0)
    cases["all_positive"] = dict(dims=dims, s=s, origin=origin, tsdf=np.ones((5, 7, 9), np.float32), weight=np.ones((5, 7, 9), np.float32),
                                 colors=None, min_weight=1.0)
    return cases


def mirror_extract(c):
    return M.extract(c["tsdf"], c["weight"], c["origin"], c["s"], c["dims"], c["min_weight"], c["colors"])


# ---- the room -----------------------------------------------------------------------------------------------------------------
# Ground-truth fusion of make_room_sequence(6, step_scale=40) at 160 x 120 into 4 cm voxels over the room's bounds.
# Truncation: 2 voxels.  An edge that crosses the surface is up to sqrt(3) voxels long and both its ends must lie inside the band to be
# observed, so 2 voxels is the narrowest band that brackets every crossing; ground-truth depth carries no noise that a wider band would
# average.  A wider band only lengthens the side walls the projective distance grows behind every occlusion boundary (the vertices
# the test exempts): the mirror measures 0.16 % exempt vertices at 2 voxels, 0.67 % at 3 and 1.29 % at the default 4 -- beyond the 1 % cap.
ROOM_INTR = dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120)
ROOM_LO, ROOM_HI, ROOM_VOXEL = (-3.0, -1.5, -3.0), (3.0, 1.5, 3.0), 0.04
ROOM_TRUNC = 2 * ROOM_VOXEL
ROOM_BOUND = ROOM_VOXEL * math.sqrt(3) / 2 + 1e-3
ROOM_EXEMPT_CAP = 0.01


def room_frames(device):
    from monogs_amd.sequences import make_room_sequence
    return make_room_sequence(6, ROOM_INTR, device=device, step_scale=40)


def room_dims():
    return tuple(int(math.ceil((h - l) / ROOM_VOXEL - 1e-6)) + 1 for l, h in zip(ROOM_LO, ROOM_HI))


def near_a_discontinuity(points, frs, intr, trunc):
    """bool [N]: the point projects, in some frame, within ``fx trunc / z + 1`` pixels of a pixel whose depth differs from a 4-neighbour's
    by more than ``trunc`` -- "within trunc of a depth discontinuity", measured sideways at the point's own depth (the + 1: a pixel is a
    square, not its centre).  ``frs``: objects with ``depth``, ``R_gt``, ``T_gt`` (torch tensors)."""
    pts = np.asarray(points, np.float64)
    near = np.zeros(len(pts), dtype=bool)
    for f in frs:
        D = f.depth.cpu().numpy().astype(np.float64)
        disc = np.zeros(D.shape, dtype=bool)
        j = np.abs(D[:, 1:] - D[:, :-1]) > trunc
        disc[:, 1:] |= j
        disc[:, :-1] |= j
        j = np.abs(D[1:] - D[:-1]) > trunc
        disc[1:] |= j
        disc[:-1] |= j
        ys, xs = np.nonzero(disc)
        pc = pts @ f.R_gt.cpu().numpy().astype(np.float64).T + f.T_gt.cpu().numpy().astype(np.float64)
        z = pc[:, 2]
        for n in np.nonzero((z > 0.01) & ~near)[0]:
            u, v = intr.fx * pc[n, 0] / z[n] + intr.cx, intr.fy * pc[n, 1] / z[n] + intr.cy
            r = intr.fx * trunc / z[n] + 1.0
            near[n] = bool((((xs + 0.5 - u) ** 2 + (ys + 0.5 - v) ** 2) <= r * r).any())
    return near


def check_room_mesh(vertices, frs, intr):
    """The assertions of the room test on a vertex array [V,3] (numpy); returns the figures."""
    import torch
    from monogs_amd.sequences import room_surface_distance
    v = np.asarray(vertices, np.float64)
    assert len(v) > 0
    d = room_surface_distance(torch.from_numpy(v)).numpy()
    far = d > ROOM_BOUND
    share = float(far.mean())
    near = near_a_discontinuity(v[far], frs, intr, ROOM_TRUNC)
    print(f"room mesh: {len(v)} vertices, {int(far.sum())} beyond {ROOM_BOUND:.4f} m ({share:.4%}), worst {d.max():.4f} m, "
          f"{int((~near).sum())} of them away from every depth discontinuity")
    assert share <= ROOM_EXEMPT_CAP, share
    assert near.all(), v[far][~near][:5]
    return dict(vertices=len(v), exempt=int(far.sum()), share=share, worst=float(d.max()))
