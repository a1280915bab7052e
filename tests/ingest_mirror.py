"""Plain numpy restatement (float64 / integers) of the frame ingest, independent of the library: the undistortion map, the
integer bilinear remap of an 8-bit image, the colour / depth conversions, the segmentation mask, the Scharr gradient intensity
and the lower median.  Written from the formulas, pixel by pixel where that is the clearest form."""
import math

import numpy as np


def undistort_map(fx, fy, cx, cy, k1, k2, p1, p2, k3, width, height):
    mx = np.empty((height, width), dtype=np.float64)
    my = np.empty((height, width), dtype=np.float64)
    for v in range(height):
        for u in range(width):
            x, y = (u - cx) / fx, (v - cy) / fy
            r2 = x * x + y * y
            kr = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            mx[v, u], my[v, u] = fx * xd + cx, fy * yd + cy
    return mx.astype(np.float32), my.astype(np.float32)


def _fixed(m):
    """round-half-even(32 m) as a Python int, None for NaN / infinity."""
    m = float(m) * 32.0
    return int(round(m)) if math.isfinite(m) else None          # Python's round() rounds halves to even


def remap_u8(src, map_x, map_y):
    """8-bit bilinear remap with 5 fractional bits, weights summing to 2^15 and a constant-zero border, in Python integers."""
    H, W, Cn = src.shape
    out = np.zeros((H, W, Cn), dtype=np.uint8)
    s = src.astype(np.int64)
    for y in range(H):
        for x in range(W):
            sx, sy = _fixed(map_x[y, x]), _fixed(map_y[y, x])
            if sx is None or sy is None:
                continue
            ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31        # Python's >> is arithmetic on negative integers
            acc = np.zeros(Cn, dtype=np.int64)
            for yy, xx, w in ((iy, ix, (32 - ax) * (32 - ay) * 32), (iy, ix + 1, ax * (32 - ay) * 32),
                              (iy + 1, ix, (32 - ax) * ay * 32), (iy + 1, ix + 1, ax * ay * 32)):
                if 0 <= yy < H and 0 <= xx < W:
                    acc += w * s[yy, xx]
            out[y, x] = (acc + 16384) >> 15
    return out


def bilinear_f64(src, map_x, map_y):
    """True bilinear interpolation in float64 where all four neighbours lie inside the image; NaN elsewhere."""
    H, W, Cn = src.shape
    out = np.full((H, W, Cn), np.nan)
    s = src.astype(np.float64)
    for y in range(H):
        for x in range(W):
            mx, my = float(map_x[y, x]), float(map_y[y, x])
            if not (math.isfinite(mx) and math.isfinite(my)):
                continue
            ix, iy = math.floor(mx), math.floor(my)
            if 0 <= ix and ix + 1 < W and 0 <= iy and iy + 1 < H:
                a, b = mx - ix, my - iy
                out[y, x] = ((1 - a) * (1 - b) * s[iy, ix] + a * (1 - b) * s[iy, ix + 1]
                             + (1 - a) * b * s[iy + 1, ix] + a * b * s[iy + 1, ix + 1])
    return out


def colour(u8_hwc):
    """[H,W,3] uint8 -> [3,H,W] float32 = float32(v / 255.0), the division in float64."""
    return np.ascontiguousarray(np.float32(u8_hwc.astype(np.float64) / 255.0).transpose(2, 0, 1))


def depth(u16, scale):
    return np.float32(u16.astype(np.float64) / float(scale))


def mask(segmentation, masked_ids):
    m = np.ones(segmentation.shape, dtype=bool)
    for i in masked_ids:
        m[segmentation == i] = False
    return m


def lower_median(values):
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    return v[(v.size - 1) // 2]


def intensity(rgb, eps=0.01):
    """[3,H,W] -> float64 [H,W]: Scharr gradient magnitude of the reflect-padded grey image, zero where a 3x3 neighbourhood
    holds |grey| <= eps."""
    g = np.asarray(rgb, dtype=np.float64).sum(axis=0) / 3.0
    p = np.pad(g, 1, mode="reflect")
    H, W = g.shape
    out = np.zeros((H, W))
    kv = np.array([[3.0, 10.0, 3.0], [0.0, 0.0, 0.0], [-3.0, -10.0, -3.0]])
    kh = kv.T
    for y in range(H):
        for x in range(W):
            n = p[y:y + 3, x:x + 3]
            if (np.abs(n) > eps).all():
                out[y, x] = math.hypot((kv * n).sum() / 32.0, (kh * n).sum() / 32.0)
    return out


def grad_mask(rgb, edge_threshold=1.1, eps=0.01):
    """(intensity, threshold, mask) in float64."""
    it = intensity(rgb, eps)
    thr = lower_median(it) * edge_threshold
    return it, thr, it > thr
