"""TEST INFRASTRUCTURE: the specification of mesh rendering ("Mesh rendering") restated in float64 numpy, brute force
over pixels x triangles, one tile of pixels at a time against the triangles a conservative box test leaves for the tile (``tile=None``:
against all of them; tests/test_mesh_render_host.py holds the two equal).  No GPU, no library.

``render`` returns depth, triangle id and colour of the specification, and two masks the GPU tests need:

* ``ambiguous``: the pixels whose hit / no-hit, or whose depth by more than ``Z_MARGIN`` metres, changes when every ``wi >= 0`` test
  is replaced by ``wi >= -+W_MARGIN (|w0| + |w1| + |w2|)`` (the *grown* and the *shrunk* test).  A float32 kernel may differ from the
  mirror there and nowhere else.
* ``unique``: the pixels where exactly one triangle of the grown test lies within ``Z_MARGIN`` of the nearest grown hit -- where the
  reported triangle cannot depend on rounding or on the order of the triangles.

All three tests come from ONE evaluation of the ``w``'s.  ``dtype=np.float32`` is the float32 restatement the GPU tolerances are
measured against (tests/test_mesh_render_host.py)."""
import numpy as np

W_MARGIN, Z_MARGIN = 1e-4, 1e-4


def camera_vertices(vertices, R, t, dtype=np.float64):
    """Camera-space vertices [V,3]: ``R v + t``, summed left to right as ``MGS_TO_CAMERA`` does."""
    v, R, t = np.asarray(vertices, dtype), np.asarray(R, dtype), np.asarray(t, dtype)
    return np.stack([R[k, 0] * v[:, 0] + R[k, 1] * v[:, 1] + R[k, 2] * v[:, 2] + t[k] for k in range(3)], 1)


def edge_vectors(vc, triangles):
    """``(E [3,T,3], z [3,T], valid [T])``: E[i] is the canonical edge vector of ``wi`` -- the cross product of the edge's endpoints in
    ascending vertex-index order, with the sign of the triangle's direction of travel (0 for a repeated index); z[i] the camera-space
    depth of vertex i.  A triangle that names a vertex outside [0, V) is invalid and all zero."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    valid = ((tri >= 0) & (tri < len(vc))).all(axis=1)
    safe = np.where(valid[:, None], tri, 0)
    E = np.zeros((3, len(tri), 3), vc.dtype)
    for i, (ja, jb) in enumerate(((1, 2), (2, 0), (0, 1))):
        ia, ib = safe[:, ja], safe[:, jb]
        swap = ia > ib
        lo, hi = vc[np.where(swap, ib, ia)], vc[np.where(swap, ia, ib)]
        c = np.cross(lo, hi).astype(vc.dtype)
        c = np.where(swap[:, None], -c, c)
        E[i] = np.where(((ia == ib) | ~valid)[:, None], 0, c)
    z = np.stack([np.where(valid, vc[safe[:, i], 2], 0) for i in range(3)])
    return E, z.astype(vc.dtype), valid


def rays(intr, dtype=np.float64):
    """[H W, 3]: pixel (px, py) looks along ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1)."""
    H, W = int(intr["H"]), int(intr["W"])
    py, px = np.mgrid[0:H, 0:W]
    half = dtype(0.5)
    dx = (px.astype(dtype) + half - dtype(intr["cx"])) / dtype(intr["fx"])
    dy = (py.astype(dtype) + half - dtype(intr["cy"])) / dtype(intr["fy"])
    return np.stack([dx, dy, np.ones_like(dx)], -1).reshape(-1, 3)


def _weights(d, E):
    """w0, w1, w2 [P,T] of the rays ``d`` [P,3]."""
    return [d[:, 0:1] * E[i][None, :, 0] + d[:, 1:2] * E[i][None, :, 1] + E[i][None, :, 2] for i in range(3)]


def _accept(z, S, near, far, two_sided):
    ok = (S != 0) & (z >= near)
    if far > 0:
        ok &= z <= far
    if not two_sided:
        ok &= S < 0
    return ok


def _candidates(vc, tri, valid, intr, near, tile):
    """Per pixel tile ``(y0, y1, x0, x1)``: the indices of the triangles that can pass the grown test somewhere in it -- every triangle
    with a vertex nearer than ``near`` or a projection beyond 1e4 pixels, and those whose projected box, grown by two pixels, meets the
    tile.  (The grown test reaches W_MARGIN of a triangle's height beyond its edges: below a pixel for every triangle that is boxed.)
    A triangle wholly nearer than ``near`` is in no tile: a hit's depth is a convex combination of the three (a 1e-3 margin for its
    rounding).  ``tile`` None: one tile, every triangle -- plain brute force."""
    H, W = int(intr["H"]), int(intr["W"])
    if tile is None:
        yield (0, H, 0, W), np.arange(len(tri))
        return
    v = vc.astype(np.float64)[np.where(valid[:, None], tri, 0)]                       # [T,3,3]
    z = v[..., 2]
    with np.errstate(all="ignore"):
        u = intr["fx"] * v[..., 0] / z + intr["cx"] - 0.5
        w = intr["fy"] * v[..., 1] / z + intr["cy"] - 0.5
    boxed = (z.min(axis=1) >= max(near, 1e-6)) & (np.abs(u).max(axis=1) < 1e4) & (np.abs(w).max(axis=1) < 1e4)
    live = z.max(axis=1) >= near * (1 - 1e-3) - 1e-12
    ulo, uhi, wlo, whi = u.min(axis=1) - 2, u.max(axis=1) + 2, w.min(axis=1) - 2, w.max(axis=1) + 2
    for y0 in range(0, H, tile):
        rows = live & (~boxed | ((whi >= y0) & (wlo <= y0 + tile - 1)))
        for x0 in range(0, W, tile):
            yield (y0, min(y0 + tile, H), x0, min(x0 + tile, W)), np.nonzero(rows & (~boxed | ((uhi >= x0) & (ulo <= x0 + tile - 1))))[0]


def render(vertices, triangles, R, t, intr, colors=None, near=0.01, far=0.0, two_sided=True, dtype=np.float64, tile=8):
    """dict(depth [H,W] (0: no hit), tri_id [H,W] (-1), rgb [3,H,W] or None (0 where nothing is hit), hit, ambiguous, unique [H,W] bool,
    status) of the specification in ``dtype``.  Pixels x triangles, one pixel tile at a time, against the triangles ``_candidates``
    keeps for the tile (``tile=None``: against all of them)."""
    dtype = np.dtype(dtype).type
    H, W = int(intr["H"]), int(intr["W"])
    vc = camera_vertices(vertices, R, t, dtype)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    E, zv, valid = edge_vectors(vc, tri)
    D = rays(intr, dtype)
    P, T = len(D), len(tri)
    inf = np.inf
    depth = np.full((3, P), inf)                       # strict, grown, shrunk
    tid = np.full(P, -1, np.int64)
    unique = np.zeros(P, bool)
    rgb = np.zeros((3, P)) if colors is not None else None
    col = np.asarray(colors, dtype) if colors is not None else None
    pix = np.arange(P).reshape(H, W)
    for (y0, y1, x0, x1), cand in (_candidates(vc, tri, valid, intr, near, tile) if T else ()):
        if not len(cand):
            continue
        sel = pix[y0:y1, x0:x1].reshape(-1)
        d, Ec, zc = D[sel], E[:, cand], zv[:, cand]
        with np.errstate(all="ignore"):
            w0, w1, w2 = _weights(d, Ec)
            S = (w0 + w1) + w2
            z = (w0 * zc[0][None] + w1 * zc[1][None] + w2 * zc[2][None]) / S
            ok = _accept(z, S, dtype(near), dtype(far), two_sided) & valid[cand][None]
            zz = np.where(ok, z, inf).astype(np.float64)
            mn, mx = np.minimum(np.minimum(w0, w1), w2), np.maximum(np.maximum(w0, w1), w2)
            eps = dtype(W_MARGIN) * (np.abs(w0) + np.abs(w1) + np.abs(w2))
            inside = [(mn >= 0) | (mx <= 0), (mn >= -eps) | (mx <= eps), (mn >= eps) | (mx <= -eps)]
        zk = [np.where(m, zz, inf) for m in inside]
        for k in range(3):
            depth[k, sel] = zk[k].min(axis=1)
        col_win = zk[0].argmin(axis=1)                  # the first of equal depths: the smallest triangle index (cand ascends)
        win = cand[col_win]
        hit = np.isfinite(depth[0, sel])
        tid[sel] = np.where(hit, win, -1)
        unique[sel] = (zk[1] <= (depth[1, sel] + Z_MARGIN)[:, None]).sum(axis=1) == 1
        if col is not None:
            rows = np.arange(len(d))
            ws = [w[rows, col_win] for w in (w0, w1, w2)]
            with np.errstate(all="ignore"):
                c = sum(ws[i][:, None] * col[np.where(valid[win], tri[win, i], 0)] for i in range(3)) / S[rows, col_win][:, None]
            rgb[:, sel] = np.where(hit[None], c.T, 0.0)
    hit = np.isfinite(depth)
    with np.errstate(invalid="ignore"):
        moved = np.abs(np.where(hit, depth, 0.0) - np.where(hit[0], depth[0], 0.0)[None]) > Z_MARGIN
    ambiguous = (hit != hit[0:1]).any(axis=0) | (moved & hit & hit[0:1]).any(axis=0)
    return dict(depth=np.where(hit[0], depth[0], 0.0).reshape(H, W), tri_id=tid.reshape(H, W),
                rgb=rgb.reshape(3, H, W) if rgb is not None else None, hit=hit[0].reshape(H, W), ambiguous=ambiguous.reshape(H, W),
                unique=(unique & hit[0]).reshape(H, W), status=0 if valid.all() else 1)


def grown_accepts(vertices, triangles, R, t, intr, tri_id, near=0.01, far=0.0, two_sided=True):
    """``(ok [H,W] bool, z [H,W])``: does the grown test accept triangle ``tri_id[y, x]`` at pixel (x, y), and at which depth (float64)."""
    H, W = int(intr["H"]), int(intr["W"])
    vc = camera_vertices(vertices, R, t)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    ids = np.asarray(tri_id, np.int64).reshape(-1)
    inside = (ids >= 0) & (ids < len(tri))
    E, zv, valid = edge_vectors(vc, tri[np.where(inside, ids, 0)])
    D = rays(intr)
    with np.errstate(all="ignore"):
        w = [D[:, 0] * E[i][:, 0] + D[:, 1] * E[i][:, 1] + E[i][:, 2] for i in range(3)]
        S = (w[0] + w[1]) + w[2]
        z = (w[0] * zv[0] + w[1] * zv[1] + w[2] * zv[2]) / S
        mn, mx = np.minimum(np.minimum(w[0], w[1]), w[2]), np.maximum(np.maximum(w[0], w[1]), w[2])
        eps = W_MARGIN * (np.abs(w[0]) + np.abs(w[1]) + np.abs(w[2]))
        ok = inside & valid & _accept(z, S, near - Z_MARGIN, far + Z_MARGIN if far > 0 else far, two_sided) & ((mn >= -eps) | (mx <= eps))
    return ok.reshape(H, W), z.reshape(H, W)


def depth_l1(a, b, max_depth=0.0):
    """The row of ``mgs_depth_l1`` in float64: sum |a - b| where both > 0 (and <= max_depth), that count, the count of b > 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    on = (a > 0) & (b > 0)
    if max_depth > 0:
        on &= (a <= max_depth) & (b <= max_depth)
    return float(np.abs(a - b)[on].sum()), int(on.sum()), int((b > 0).sum())
