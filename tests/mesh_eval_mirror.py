"""TEST INFRASTRUCTURE: the specification of the reconstruction evaluation ("Reconstruction evaluation") restated in
float64 numpy, with scipy's cKDTree for the nearest neighbour.  Nothing here runs on the GPU or imports the native library."""
import math

import numpy as np
from scipy.spatial import cKDTree


# ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
def nn_brute(queries, targets):
    """(d2 [Q] float64, index [Q]) by brute force in float64; the smallest index among equal distances.  No targets: inf, -1."""
    q, t = np.asarray(queries, np.float64), np.asarray(targets, np.float64)
    if len(t) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1, np.int64)
    d2 = np.empty(len(q))
    idx = np.empty(len(q), np.int64)
    step = max(1, (1 << 22) // max(len(t), 1))
    for s in range(0, len(q), step):
        d = ((q[s:s + step, None, :] - t[None, :, :]) ** 2).sum(-1)
        idx[s:s + step] = d.argmin(1)                               # argmin: the first (smallest) index of the minimum
        d2[s:s + step] = d[np.arange(d.shape[0]), idx[s:s + step]]
    return d2, idx


def nn_tree(queries, targets):
    """d2 [Q] float64 by cKDTree."""
    q, t = np.asarray(queries, np.float64), np.asarray(targets, np.float64)
    if len(t) == 0:
        return np.full(len(q), np.inf)
    d, _ = cKDTree(t).query(q)
    return d * d


# ---- sampling -------------------------------------------------------------------------------------------------------------------
def _mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def uniforms(seed, n):
    """[n,3] float64: the three uniforms of samples 0..n-1 (24 bits each)."""
    with np.errstate(over="ignore"):
        h0 = _mix(np.array([(seed & 0xFFFFFFFF) ^ 0x9E3779B9], np.uint32))[0] + np.uint32(3) * np.arange(n, dtype=np.uint32)
        return np.stack([(_mix(h0 + np.uint32(k)) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 for k in range(3)], 1)


def area_scale(vertices, n_triangles):
    """The power of two the float32 areas are quantised by: 2^(61 - eT - eD), the squared bounding-box diagonal D2 < 2^eD (float64 of
    the float32 bounds) and T <= 2^eT."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    ext = v.max(0) - v.min(0)
    d2 = float((ext * ext)[0] + (ext * ext)[1] + (ext * ext)[2])
    eD = math.frexp(d2)[1] if d2 > 0 else 0
    eT = 0
    while (1 << eT) < n_triangles:
        eT += 1
    return math.ldexp(1.0, 61 - eT - eD)


def areas_f32(vertices, triangles):
    """float32 areas 0.5 |(b - a) x (c - a)|, every operation rounded to float32 (the order of the three-term sum is the kernel's)."""
    v, t = np.asarray(vertices, np.float32), np.asarray(triangles, np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = np.cross((b - a).astype(np.float32), (c - a).astype(np.float32)).astype(np.float32)
    return (np.float32(0.5) * np.sqrt((n * n).sum(1, dtype=np.float32), dtype=np.float32)).astype(np.float32)


def sample(vertices, triangles, n, seed, keep=None, areas=None):
    """(points [n,3] float64, tri [n], kept area): the rule on the given float32 ``areas`` (default: ``areas_f32``)."""
    v, t = np.asarray(vertices, np.float32).astype(np.float64), np.asarray(triangles, np.int64)
    ar = areas_f32(vertices, triangles) if areas is None else np.asarray(areas, np.float32)
    if keep is not None:
        ar = np.where(np.asarray(keep) != 0, ar, np.float32(0))
    scale = area_scale(vertices, len(t))
    q = np.floor(ar.astype(np.float64) * scale).astype(np.uint64)
    incl = np.cumsum(q, dtype=np.uint64)
    total = int(incl[-1])
    r = uniforms(seed, n)
    x = (np.arange(n, dtype=np.float64) + r[:, 0]) / float(n) * float(np.float64(np.uint64(total)))
    u = np.minimum(x.astype(np.uint64), np.uint64(total - 1))
    tri = np.searchsorted(incl, u, side="right")                    # the first triangle whose inclusive sum exceeds u
    a, b, c = v[t[tri, 0]], v[t[tri, 1]], v[t[tri, 2]]
    su = np.sqrt(r[:, 1])
    p = a + (su * (1 - r[:, 2]))[:, None] * (b - a) + (su * r[:, 2])[:, None] * (c - a)
    return p, tri, total / scale


# ---- visibility -----------------------------------------------------------------------------------------------------------------
def seen(vertices, R, t, fx, fy, cx, cy, W, H, depth=None, depth_min=0.01, depth_max=0.0, eps=0.03):
    """(seen [V] bool, pixel margin [V], metric margin [V]): the rule in float64, and how far each decision is from flipping -- the
    distance of the projection to the nearest pixel border in pixels and of z to the nearest of its limits in metres (inf where a
    limit does not apply)."""
    p = np.asarray(vertices, np.float64)
    pc = p @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    z = pc[:, 2]
    ok = (z > 0) & (z >= depth_min)
    m_m = np.abs(z - max(depth_min, 0.0))
    if depth_max > 0:
        ok &= z <= depth_max
        m_m = np.minimum(m_m, np.abs(z - depth_max))
    zs = np.where(z > 0, z, 1.0)
    u, v = fx * pc[:, 0] / zs + cx - 0.5, fy * pc[:, 1] / zs + cy - 0.5
    fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
    m_px = np.minimum(np.abs(u + 0.5 - np.round(u + 0.5)), np.abs(v + 0.5 - np.round(v + 0.5)))
    inside = (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    ok &= inside
    if depth is not None:
        D = np.asarray(depth, np.float64)
        d = D[np.clip(fv, 0, H - 1).astype(int), np.clip(fu, 0, W - 1).astype(int)]
        ok &= (d > 0) & (z <= d + eps)
        m_m = np.where(inside & (d > 0), np.minimum(m_m, np.abs(d + eps - z)), m_m)
    return ok, m_px, m_m


# ---- figures --------------------------------------------------------------------------------------------------------------------
def metrics(d2, thresholds):
    """[2 + K] float64: sum of sqrt(d2) over the finite entries, their number, the number below each threshold."""
    d2 = np.asarray(d2, np.float32).astype(np.float64)
    d = np.sqrt(d2[np.isfinite(d2)])
    return np.array([d.sum(), len(d)] + [float((d < float(np.float32(th))).sum()) for th in thresholds])


def figures(d2_acc, d2_comp, threshold):
    a, c = metrics(d2_acc, [threshold]), metrics(d2_comp, [threshold])
    accuracy, completion = a[0] / a[1], c[0] / c[1]
    precision, recall = a[2] / a[1], c[2] / c[1]
    return dict(accuracy_m=accuracy, completion_m=completion, completion_ratio=recall, chamfer_l1_m=0.5 * (accuracy + completion),
                precision=precision, recall=recall, fscore=2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0)


def eval_meshes(rec_v, rec_t, gt_v, gt_t, n, threshold=0.05, seed=0):
    """The whole protocol in float64 on the mirror's own samples (seeds ``seed`` and ``seed + 1``)."""
    pr, _, ar = sample(rec_v, rec_t, n, seed)
    pg, _, ag = sample(gt_v, gt_t, n, seed + 1)
    out = figures(nn_tree(pr, pg), nn_tree(pg, pr), threshold)
    out.update(rec_area_m2=ar, gt_area_m2=ag)
    return out
