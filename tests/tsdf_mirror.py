"""TEST INFRASTRUCTURE: a float64 numpy restatement of DESIGN.md, "TSDF fusion and mesh extraction" (csrc/tsdf.hip).

``integrate`` applies one frame to float64 planes and returns, per voxel, how far each of its decisions was from flipping (the
*margin*): a float32 kernel may decide a voxel whose margin is below its rounding error the other way, and the tests exempt
exactly those.  ``extract`` produces the mesh in the defined orders (vertices by (owner index, edge bit), triangles by (cell
index, tetrahedron, triangle)), so index buffers compare exactly.  The sign cases of a tetrahedron are derived here from the
corner coordinates (determinants), not from the kernel's table."""
import itertools

import numpy as np

# owned edge bits 0..6: +x, +y, +z, +x+y, +y+z, +x+z, +x+y+z
EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))            # lexicographic: tetrahedron t walks 000 -> +a -> +a+b -> 111


def new_planes(dims, color=True):
    nx, ny, nz = dims
    p = np.zeros((5 if color else 2, nz, ny, nx), dtype=np.float64)
    p[0] = 1.0
    return p


def voxel_centres(origin, s, dims):
    """[nz, ny, nx, 3] float64 of the float32 centres the kernel forms (origin + s * index in float32)."""
    nx, ny, nz = dims
    o, s = np.asarray(origin, np.float32), np.float32(s)
    x = (o[0] + s * np.arange(nx, dtype=np.float32)).astype(np.float64)
    y = (o[1] + s * np.arange(ny, dtype=np.float32)).astype(np.float64)
    z = (o[2] + s * np.arange(nz, dtype=np.float32)).astype(np.float64)
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx, yy, zz], -1)


def integrate(planes, origin, s, dims, depth, R, t, fx, fy, cx, cy, trunc, depth_min=0.01, depth_max=0.0, opacity=None,
              opacity_min=0.9, rgb=None, max_weight=64.0):
    """Updates ``planes`` in place.  Returns ``(visited [nz,ny,nx] bool, margin_px, margin_m)``: the voxels that reached the update,
    the distance of u + 0.5 / v + 0.5 to the nearest integer (pixels) and the smallest distance of pc.z to depth_min, of sdf to
    -trunc, of d to depth_min and depth_max and of the opacity to opacity_min (metres / opacity units); +inf for a decision
    the voxel never reached."""
    f64 = lambda a: np.asarray(np.asarray(a, np.float32), np.float64)  # noqa: E731  (the float32 inputs the kernel sees)
    depth, R, t = f64(depth), f64(R), f64(t)
    fx, fy, cx, cy, trunc, depth_min, depth_max, opacity_min, max_weight = (float(np.float32(v)) for v in (
        fx, fy, cx, cy, trunc, depth_min, depth_max, opacity_min, max_weight))
    H, W = depth.shape
    p = voxel_centres(origin, s, dims)
    pc = p @ R.T + t
    z = pc[..., 2]
    inf = np.full(z.shape, np.inf)
    margin_m = np.abs(z - depth_min)
    live = z > depth_min
    zs = np.where(live, z, 1.0)
    u5, v5 = fx * pc[..., 0] / zs + cx, fy * pc[..., 1] / zs + cy           # u + 0.5, v + 0.5
    margin_px = np.where(live, np.minimum(np.abs(u5 - np.round(u5)), np.abs(v5 - np.round(v5))), inf)
    ix, iy = np.floor(u5), np.floor(v5)
    live &= (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    ixc, iyc = np.clip(ix, 0, W - 1).astype(np.int64), np.clip(iy, 0, H - 1).astype(np.int64)
    d = depth[iyc, ixc]
    if opacity is not None:
        a = f64(opacity)[iyc, ixc]
        margin_m = np.minimum(margin_m, np.where(live, np.abs(a - opacity_min), inf))
        live &= a >= opacity_min
        d = d / np.where(live, a, 1.0)
    margin_m = np.minimum(margin_m, np.where(live, np.abs(d - depth_min), inf))
    if depth_max > 0:
        margin_m = np.minimum(margin_m, np.where(live, np.abs(d - depth_max), inf))
    live &= (d > depth_min) & ((depth_max <= 0) | (d <= depth_max))
    sdf = d - z
    margin_m = np.minimum(margin_m, np.where(live, np.abs(sdf + trunc), inf))
    live &= sdf >= -trunc
    f = np.minimum(1.0, sdf / trunc)
    w = planes[1]
    planes[0] = np.where(live, (planes[0] * w + f) / (w + 1.0), planes[0])
    if rgb is not None and planes.shape[0] == 5:
        rgb = f64(rgb)
        for c in range(3):
            planes[2 + c] = np.where(live, (planes[2 + c] * w + rgb[c][iyc, ixc]) / (w + 1.0), planes[2 + c])
    planes[1] = np.where(live, np.minimum(w + 1.0, max_weight), w)
    return live, margin_px, margin_m


def _shift(a, dx, dy, dz, fill):
    """out[k, j, i] = a[k + dz, j + dy, i + dx] where that exists, ``fill`` elsewhere (offsets in -1, 0, 1)."""
    out = np.full(a.shape, fill, dtype=a.dtype)
    nz, ny, nx = a.shape

    def sl(n, d):
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
    (kz, sz), (ky, sy), (kx, sx) = sl(nz, dz), sl(ny, dy), sl(nx, dx)
    out[kz, ky, kx] = a[sz, sy, sx]
    return out


def _tet_cases(t):
    """{mask: [(edge, edge, edge), ...]} for tetrahedron ``t``; an edge is (owner corner offset (dx,dy,dz), bit).  Bit n of the mask:
    vertex n inside.  The first edge of a triangle is fixed by the rule below; the other two are ordered so that the normal
    points towards the outside (positive) vertices -- decided by determinants of the corner coordinates.
      one vertex p apart, the others q0 < q1 < q2: edges (p q0), (p q1), (p q2);
      two inside p < q, two outside r < s: A = (p r), B = (p s), C = (q s), D = (q r): triangles (A, B, C), (A, C, D)."""
    a, b, c = PERMS[t]
    P = np.zeros((4, 3), dtype=np.int64)
    P[1, a] = 1
    P[2] = P[1]
    P[2, b] = 1
    P[3] = 1

    def edge(p, q):
        lo, hi = min(p, q), max(p, q)
        return (tuple(int(x) for x in P[lo]), EDGE_DIRS.index(tuple(int(x) for x in P[hi] - P[lo])))

    cases = {}
    for m in range(1, 15):
        ins = [n for n in range(4) if (m >> n) & 1]
        out = [n for n in range(4) if not (m >> n) & 1]
        if len(ins) in (1, 3):
            p, q = (ins[0], out) if len(ins) == 1 else (out[0], ins)
            det = np.linalg.det((P[q] - P[p]).astype(np.float64))        # > 0: (q0, q1, q2) seen from p is counter-clockwise
            away = det > 0                                               # the normal of (q0, q1, q2) points away from p
            keep = away if len(ins) == 1 else not away
            q1, q2 = (q[1], q[2]) if keep else (q[2], q[1])
            cases[m] = [(edge(p, q[0]), edge(p, q1), edge(p, q2))]
        else:
            (p, q), (r, s) = ins, out
            A, B, Cc, D = edge(p, r), edge(p, s), edge(q, s), edge(q, r)
            det = np.linalg.det(np.stack([P[q] - P[p], P[r] - P[p], P[s] - P[p]]).astype(np.float64))
            cases[m] = [(A, B, Cc), (A, Cc, D)] if det > 0 else [(A, Cc, B), (A, D, Cc)]
    return cases, P


def extract(tsdf, weight, origin, s, dims, min_weight=1.0, colors=None):
    """``tsdf``, ``weight`` [nz,ny,nx] (the float32 values the kernel sees), ``colors`` [3,nz,ny,nx] or None.  Returns
    ``dict(vertices [V,3] f64, colors [V,3] f64 or None, triangles [T,3] int64, valid [nz,ny,nx] bool, edge_mask [nz,ny,nx] uint8)``."""
    nx, ny, nz = dims
    tsdf = np.asarray(np.asarray(tsdf, np.float32), np.float64).reshape(nz, ny, nx)
    weight = np.asarray(np.asarray(weight, np.float32), np.float64).reshape(nz, ny, nx)
    obs, ins = weight >= float(np.float32(min_weight)), tsdf < 0
    valid = np.ones((nz, ny, nx), dtype=bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        valid &= _shift(obs, dx, dy, dz, False)                        # a corner beyond the grid: no cell
    has = np.zeros((nz, ny, nx, 7), dtype=bool)
    for e, (dx, dy, dz) in enumerate(EDGE_DIRS):
        other_in = _shift(ins, dx, dy, dz, False)
        other_ok = _shift(np.ones_like(obs), dx, dy, dz, False)        # the far end exists
        contained = np.zeros_like(valid)
        for ca in ((0,) if dx else (0, 1)):
            for cb in ((0,) if dy else (0, 1)):
                for cc in ((0,) if dz else (0, 1)):
                    contained |= _shift(valid, -ca, -cb, -cc, False)
        has[..., e] = other_ok & obs & _shift(obs, dx, dy, dz, False) & (ins != other_in) & contained
    vid = np.cumsum(has.reshape(-1)).reshape(nz, ny, nx, 7) - 1        # (owner linear index, bit) order
    p = voxel_centres(origin, s, dims)
    s64 = float(np.float32(s))
    verts, cols = [], []
    col = None if colors is None else np.asarray(np.asarray(colors, np.float32), np.float64).reshape(3, nz, ny, nx)
    order = []
    for e, (dx, dy, dz) in enumerate(EDGE_DIRS):
        k, j, i = np.nonzero(has[..., e])
        fa, fb = tsdf[k, j, i], tsdf[k + dz, j + dy, i + dx]
        tt = fa / (fa - fb)
        verts.append(p[k, j, i] + tt[:, None] * (s64 * np.array([dx, dy, dz], dtype=np.float64)))
        if col is not None:
            ca, cb = col[:, k, j, i].T, col[:, k + dz, j + dy, i + dx].T
            cols.append(ca + tt[:, None] * (cb - ca))
        order.append(vid[k, j, i, e])
    order = np.concatenate(order) if order else np.zeros(0, np.int64)
    V = int(has.sum())
    vertices = np.zeros((V, 3))
    vertices[order] = np.concatenate(verts) if V else np.zeros((0, 3))
    vcol = None
    if col is not None:
        vcol = np.zeros((V, 3))
        vcol[order] = np.concatenate(cols) if V else np.zeros((0, 3))
    # triangles
    rows = []
    ck, cj, ci = np.nonzero(valid)
    cell = (ck * ny + cj) * nx + ci
    for t in range(6):
        cases, P = _tet_cases(t)
        m = np.zeros(cell.shape, dtype=np.int64)
        for n in range(4):
            m |= ins[ck + P[n, 2], cj + P[n, 1], ci + P[n, 0]].astype(np.int64) << n
        for mask, tris in cases.items():
            sel = m == mask
            if not sel.any():
                continue
            k, j, i = ck[sel], cj[sel], ci[sel]
            for n, tri in enumerate(tris):
                idx = [vid[k + o[2], j + o[1], i + o[0], bit] for (o, bit) in tri]
                for (o, bit) in tri:
                    assert has[k + o[2], j + o[1], i + o[0], bit].all()
                rows.append(np.stack([cell[sel], np.full(k.shape, t), np.full(k.shape, n)] + idx, axis=1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        triangles = rows[:, 3:].astype(np.int64)
    else:
        triangles = np.zeros((0, 3), dtype=np.int64)
    emask = (has.astype(np.uint8) << np.arange(7, dtype=np.uint8)).sum(-1).astype(np.uint8)
    return dict(vertices=vertices, colors=vcol, triangles=triangles, valid=valid, edge_mask=emask)


def mesh_checks(vertices, triangles):
    """``dict(closed, euler, volume, boundary, non_manifold)``: closed = every undirected edge is in exactly two triangles, once in
    each direction; euler = V - E + F; volume = the signed volume (positive: outward normals)."""
    t = np.asarray(triangles, np.int64)
    V = int(np.asarray(vertices).shape[0])
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = d.min(1) * max(V, 1) + d.max(1)
    sign = np.where(d[:, 0] < d[:, 1], 1, -1)
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    bal = np.zeros(uniq.shape, dtype=np.int64)
    np.add.at(bal, inv, sign)
    v = np.asarray(vertices, np.float64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    vol = float((a * np.cross(b - a, c - a)).sum() / 6.0)
    return dict(closed=bool((cnt == 2).all() and (bal == 0).all()), euler=V - len(uniq) + t.shape[0], volume=vol,
                boundary=int((cnt == 1).sum()), non_manifold=int((cnt > 2).sum()), edges=len(uniq))
