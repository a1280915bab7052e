"""Restatements the viewer tests compare against: the integer line rule (NORMATIVE: ``include/monogs_raster.h`` describes it, this
is it in plain Python integers), the compose rules in numpy as the reference's lines state them, the host-side clip / project /
quantise in float64 and the ellipsoid pick in float64.  Nothing here imports ``monogs_amd.viewer``."""
import math

import numpy as np

SUB = 16            # sub-pixel units per pixel; pixel centres at multiples of 16


# ---- lines ---------------------------------------------------------------------------------------------------------------------
def _floor_div(a: int, b: int) -> int:
    return a // b                      # Python's // floors


def segment_pixels(x0, y0, x1, y1):
    """The pixels (x, y) a segment paints, before clipping to the image.  Major axis: the larger extent, x on a tie; every integer
    pixel position on it inside the segment, minor coordinate rounded half up; none such: the pixel endpoint 0 rounds to."""
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    xmajor = abs(x1 - x0) >= abs(y1 - y0)
    m0, m1, n0, n1 = (x0, x1, y0, y1) if xmajor else (y0, y1, x0, x1)
    if m0 > m1:
        m0, m1, n0, n1 = m1, m0, n1, n0
    dm = m1 - m0
    lo, hi = -_floor_div(-m0, SUB), _floor_div(m1, SUB)
    if dm == 0 or lo > hi:
        return [(_floor_div(x0 + SUB // 2, SUB), _floor_div(y0 + SUB // 2, SUB))]
    out = []
    for m in range(lo, hi + 1):
        n = _floor_div(n0 * dm + (n1 - n0) * (SUB * m - m0) + (SUB // 2) * dm, SUB * dm)
        out.append((m, n) if xmajor else (n, m))
    return out


def lines_owner(segments, W, H):
    """int32 [H, W]: highest index + 1 of the segments painting each pixel, 0 where none does."""
    owner = np.zeros((H, W), dtype=np.int32)
    for s, seg in enumerate(np.asarray(segments).reshape(-1, 4)):
        for x, y in segment_pixels(*seg):
            if 0 <= x < W and 0 <= y < H:
                owner[y, x] = max(owner[y, x], s + 1)
    return owner


# ---- host side: clip, project, quantise (float64) --------------------------------------------------------------------------------
def project_segment(p, q, R, T, k, near=0.2, guard=1024.0):
    """One world-space segment -> (x0, y0, x1, y1) in 1/16 pixel, or None: clip against z >= near, project with
    ``((ndc + 1) S - 1) / 2``, clip to the image grown by ``guard`` pixels (parametrically, along the projected segment), round
    half up."""
    R, T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)
    p, q = R @ np.asarray(p, dtype=np.float64) + T, R @ np.asarray(q, dtype=np.float64) + T
    if p[2] < near and q[2] < near:
        return None
    if p[2] < near:
        p = p + (p[2] - near) / (p[2] - q[2]) * (q - p)
    elif q[2] < near:
        q = p + (p[2] - near) / (p[2] - q[2]) * (q - p)
    W, H = float(k["W"]), float(k["H"])

    def pix(v):
        nx = (2.0 * k["fx"] / W) * v[0] / v[2] + (2.0 * k["cx"] - W) / W
        ny = (2.0 * k["fy"] / H) * v[1] / v[2] + (2.0 * k["cy"] - H) / H
        return np.array([((nx + 1.0) * W - 1.0) * 0.5, ((ny + 1.0) * H - 1.0) * 0.5])

    a, b = pix(p), pix(q)
    lo, hi = 0.0, 1.0
    for fa, fb in ((a[0] + guard, b[0] + guard), (W + guard - a[0], W + guard - b[0]), (a[1] + guard, b[1] + guard),
                   (H + guard - a[1], H + guard - b[1])):
        if fa < 0.0 and fb < 0.0:
            return None
        if fa < 0.0:
            lo = max(lo, fa / (fa - fb))
        elif fb < 0.0:
            hi = min(hi, fa / (fa - fb))
    if lo > hi:
        return None
    a, b = (a if lo == 0.0 else a + lo * (b - a)), (b if hi == 1.0 else a + hi * (b - a))      # (an unclipped end stays exact)
    return tuple(math.floor(v * SUB + 0.5) for v in (a[0], a[1], b[0], b[1]))


def frustum_points(c2w, k, size=1.0):
    """gui_utils.py:69-86: the apex and the corners (W, 0), (0, 0), (W, H), (0, H) at depth max(fx, fy) * 1e-3, times size, in the world."""
    pts = [np.zeros(3)]
    Z = max(k["fx"], k["fy"]) * 1e-3
    for u, v in ((k["W"], 0.0), (0.0, 0.0), (k["W"], k["H"]), (0.0, k["H"])):
        pts.append(np.array([(u - k["cx"]) * Z / k["fx"], (v - k["cy"]) * Z / k["fy"], Z]))
    pts = np.stack(pts) * size
    c2w = np.asarray(c2w, dtype=np.float64)
    return pts @ c2w[:3, :3].T + c2w[:3, 3]


# ---- compose ---------------------------------------------------------------------------------------------------------------------
def jet_index(x):
    """matplotlib's index of a float image: clamp(floor(x * 256), 0, 255); -1 for a NaN."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        f = np.floor(x * np.float32(256.0))
        idx = np.clip(np.where(np.isnan(f), 0.0, f), 0, 255).astype(np.int64)
    return np.where(np.isnan(x), -1, idx)


def compose(mode, src, lut=None, owner=None, seg_rgb=None):
    """uint8 [H, W, 3] by the reference's lines (viewer/slam_viewer.py): rgb / segmentation :767-768 ``clip(c, 0, 1) * 255`` then
    ``.byte()``; depth :607-618 ``depth / depth.max()`` unless the maximum is 0, then jet; time :624-636 jet of the opacity image;
    elipsoids: GL's float -> unorm8 conversion ``floor(clip(c) * 255 + 0.5)``.  All in float32, as the reference computes them."""
    src = np.asarray(src, dtype=np.float32)
    if mode in ("rgb", "segmentation"):
        out = (np.clip(src, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0)
    elif mode == "elipsoids":
        out = np.floor(np.clip(src, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8).transpose(1, 2, 0)
    else:
        x = src
        if mode == "depth":
            mx = np.float32(src.max())
            if mx != 0:
                x = src / mx
        k = jet_index(x)
        out = np.where((k >= 0)[..., None], np.asarray(lut)[np.maximum(k, 0)], 0).astype(np.uint8)
    out = np.ascontiguousarray(out)
    if owner is not None and seg_rgb is not None and len(seg_rgb):
        m = owner > 0
        out[m] = np.asarray(seg_rgb)[owner[m] - 1]
    return out


# ---- ellipsoid pick (float64) ------------------------------------------------------------------------------------------------------
def ellipsoid_pick(rec, visible, W, H, threshold=0.4):
    """Per pixel, the qualifying visible Gaussian that is first by (float32 depth bits, index).  ``rec`` [P, 16] float32: the blend
    records (px, py, ., ., ka, kb, kc, opacity, r, g, b, depth, ...; (ka, kb, kc) the conic in log2 units, csrc/common.h).
    Qualifying: power <= 0 and min(0.99, opacity exp(power)) > threshold.  Returns ``hit`` int32 [H, W] (-1: none), ``color``
    float64 [3, H, W] = colour exp(power) and ``aside`` bool [H, W]: pixels whose decision hangs on rounding -- a candidate's alpha
    within 1e-4 of the threshold, its power within 1e-6 of 0, or the two front candidates' depths within 1e-5 relative."""
    rec = np.asarray(rec, dtype=np.float32)
    ids = np.nonzero(np.asarray(visible))[0]
    r = rec[ids].astype(np.float64)
    bits = rec[ids, 11].copy().view(np.uint32).astype(np.int64)
    order = np.lexsort((ids, bits))                   # by depth bits, then index
    ids, r = ids[order], r[order]
    ys, xs = np.mgrid[0:H, 0:W]
    dx = r[:, 0][:, None, None] - xs[None]
    dy = r[:, 1][:, None, None] - ys[None]
    p2 = r[:, 4][:, None, None] * dx * dx + r[:, 5][:, None, None] * dx * dy + r[:, 6][:, None, None] * dy * dy     # log2 units
    power = p2 * math.log(2.0)
    G = np.exp2(np.minimum(p2, 60.0))
    raw = r[:, 7][:, None, None] * G
    alpha = np.minimum(0.99, raw)
    qual = (power <= 0.0) & (alpha > threshold)
    n = len(ids)
    if n == 0:
        return np.full((H, W), -1, np.int32), np.zeros((3, H, W)), np.zeros((H, W), bool)
    first = np.where(qual.any(0), qual.argmax(0), n)
    hit = np.where(first < n, ids[np.minimum(first, n - 1)], -1).astype(np.int32)
    Gf = np.take_along_axis(G, np.minimum(first, n - 1)[None], 0)[0]
    color = np.where(first[None] < n, r[np.minimum(first, n - 1)][..., 8:11].transpose(2, 0, 1) * Gf[None], 0.0)
    # what hangs on rounding: only entries at or in front of the pick can change it
    pos = np.arange(n)[:, None, None]
    front = pos <= first[None]
    near_thr = (np.abs(alpha - threshold) < 1e-4) & (power <= 1e-6)
    near_zero = (np.abs(power) < 1e-6) & (raw > threshold - 1e-4)
    aside = ((near_thr | near_zero) & front).any(0)
    # the two front candidates: the pick and the next qualifying one behind it
    q2 = qual & (pos > first[None])
    second = np.where(q2.any(0), q2.argmax(0), n)
    d = r[:, 11]
    d1, d2 = d[np.minimum(first, n - 1)], d[np.minimum(second, n - 1)]
    aside |= (first < n) & (second < n) & (np.abs(d2 - d1) <= 1e-5 * np.maximum(np.abs(d1), np.abs(d2)))
    return hit, color, aside
