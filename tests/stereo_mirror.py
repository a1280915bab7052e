"""Vectorised numpy restatement, in 64-bit integers, of the stereo depth specification (include/monogs_raster.h,
mgs_stereo_depth): rectification, pre-filter, Birchfield-Tomasi pixel cost ``pc``, window sums ``C``, the five aggregation paths
``S``, winner selection with the right-view table, left-right check, 3x3 median ``disp16`` and ``depth``.  Independent of the
library; written from the formulas, step by step in the header's numbering."""
import numpy as np

EUROC_BF = 47.90639384423901
INF = np.int64(1) << 40


def defaults(block_size=20, p1=0, p2=0, uniqueness_ratio=40, disp12_max_diff=0, pre_filter_cap=0):
    """OpenCV's parameter defaulting -> dict(s, P1, P2, uniq, max_diff, ftzero)."""
    block = block_size if block_size > 0 else 5
    P1 = p1 if p1 > 0 else 2
    P2 = max(p2 if p2 > 0 else 5, P1 + 1)
    return dict(s=block // 2, P1=P1, P2=P2, uniq=uniqueness_ratio if uniqueness_ratio >= 0 else 10,
                max_diff=disp12_max_diff if disp12_max_diff > 0 else 1, ftzero=max(pre_filter_cap, 15) | 1)


# ---- step 0 ------------------------------------------------------------------------------------------------------------------
def remap_gray(src, map_x, map_y):
    """8-bit bilinear remap of one channel: 1/32-pixel coordinates (round half to even of 32 m, computed in float32 as the
    kernel does), weights summing to 2^15, constant-zero border; a non-finite or far-off coordinate gives 0."""
    H, W = src.shape
    s = src.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.rint(map_x.astype(np.float32) * np.float32(32.0))
        fy = np.rint(map_y.astype(np.float32) * np.float32(32.0))
        ok = (fx >= -32.0) & (fx < 32.0 * W) & (fy >= -32.0) & (fy < 32.0 * H)          # NaN fails
    sx = np.where(ok, fx, 0).astype(np.int64)
    sy = np.where(ok, fy, 0).astype(np.int64)
    ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31
    acc = np.full(src.shape, 16384, dtype=np.int64)
    for yy, xx, w in ((iy, ix, (32 - ax) * (32 - ay) * 32), (iy, ix + 1, ax * (32 - ay) * 32),
                      (iy + 1, ix, (32 - ax) * ay * 32), (iy + 1, ix + 1, ax * ay * 32)):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        acc += np.where(inside, w * s[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)
    return np.where(ok, acc >> 15, 0).astype(np.uint8)


def rgb(gray_u8):
    c = np.float32(gray_u8.astype(np.float64) / 255.0)
    return np.stack([c, c, c])


# ---- steps 1, 2 --------------------------------------------------------------------------------------------------------------
def prefilter(img, ftzero):
    I = img.astype(np.int64)
    H, W = I.shape
    rows = np.pad(I, ((1, 1), (0, 0)), mode="edge")
    cols = np.pad(rows, ((0, 0), (1, 1)), mode="edge")            # (the padded columns only feed x = 0, W - 1: overwritten)
    dx = cols[:, 2:] - cols[:, :-2]                                # [H + 2, W]: I[.][x + 1] - I[.][x - 1]
    g = dx[:-2] + 2 * dx[1:-1] + dx[2:]
    P = np.clip(g, -ftzero, ftzero) + ftzero
    P[:, 0] = ftzero
    P[:, W - 1] = ftzero
    return P


def _interval(J):
    p = np.pad(J, ((0, 0), (1, 1)), mode="edge")
    ul, ur = (J + p[:, :-2]) // 2, (J + p[:, 2:]) // 2
    return J, np.minimum(np.minimum(ul, ur), J), np.maximum(np.maximum(ul, ur), J)


def pc(left, right, D, ftzero):
    """Pixel cost, int64 [H, W - D, D]."""
    H, W = left.shape
    out = np.zeros((H, W - D, D), dtype=np.int64)
    xs = np.arange(D, W)
    for Jl, Jr in ((prefilter(left, ftzero), prefilter(right, ftzero)), (left.astype(np.int64), right.astype(np.int64))):
        u, u0, u1 = (a[:, xs] for a in _interval(Jl))
        v_all, v0_all, v1_all = _interval(Jr)
        for d in range(D):
            v, v0, v1 = v_all[:, xs - d], v0_all[:, xs - d], v1_all[:, xs - d]
            c0 = np.maximum(0, np.maximum(u - v1, v0 - u))
            c1 = np.maximum(0, np.maximum(v - u1, u0 - v))
            out[:, :, d] += np.minimum(c0, c1)
    return out


# ---- step 3 ------------------------------------------------------------------------------------------------------------------
def window(pcv, s):
    """C: sums over the (2s+1)^2 window with clamped rows and valid columns."""
    H, W1, _ = pcv.shape
    p = np.pad(pcv, ((s, s), (s, s), (0, 0)), mode="edge")
    out = np.zeros_like(pcv)
    for dy in range(2 * s + 1):
        for dx in range(2 * s + 1):
            out += p[dy:dy + H, dx:dx + W1]
    return out


# ---- step 4 ------------------------------------------------------------------------------------------------------------------
def _step(Cp, Lq, P1, P2):
    """One step of the recurrence for a batch of pixels: Cp, Lq [N, D]."""
    m = Lq.min(axis=1, keepdims=True)
    lo = np.concatenate([np.full_like(Lq[:, :1], INF), Lq[:, :-1]], axis=1) + P1
    hi = np.concatenate([Lq[:, 1:], np.full_like(Lq[:, :1], INF)], axis=1) + P1
    return Cp + np.minimum(np.minimum(Lq, m + P2), np.minimum(lo, hi)) - m


def aggregate(Cv, P1, P2):
    """S = the sum of L_r over the five directions, int64 [H, W1, D]."""
    H, W1, D = Cv.shape
    S = np.zeros_like(Cv)
    for xs in (range(W1), range(W1 - 1, -1, -1)):                  # from the left, from the right
        L = np.zeros((H, D), dtype=np.int64)                       # the predecessor outside the region: L = 0
        for x in xs:
            L = _step(Cv[:, x], L, P1, P2)
            S[:, x] += L
    for dx in (1, 0, -1):                                          # from up-left, above, up-right: predecessor (x - dx, y - 1)
        L = np.zeros((W1, D), dtype=np.int64)
        for y in range(H):
            Lq = np.zeros_like(L)
            if y > 0:
                if dx == 1:
                    Lq[1:] = L[:-1]
                elif dx == -1:
                    Lq[:-1] = L[1:]
                else:
                    Lq = L
            L = _step(Cv[y], Lq, P1, P2)
            S[y] += L
    return S


# ---- steps 5 .. 8 ------------------------------------------------------------------------------------------------------------
def winner(Sv, W, uniq):
    """(d16 [H, W] before the left-right check, disp2 [H, W]): step 5, the table filled in the sequential order."""
    H, W1, D = Sv.shape
    best = Sv.argmin(axis=2)                                       # the first (lowest) minimiser
    minS = Sv.min(axis=2)
    d = np.arange(D)[None, None, :]
    invalid = ((Sv * (100 - uniq) < minS[..., None] * 100) & (np.abs(best[..., None] - d) > 1)).any(axis=2)
    take = lambda k: np.take_along_axis(Sv, np.clip(k, 0, D - 1)[..., None], axis=2)[..., 0]      # noqa: E731
    sm, sp = take(best - 1), take(best + 1)
    den = np.maximum(sm + sp - 2 * minS, 1)
    num = (sm - sp) * 16 + den
    delta = np.sign(num) * (np.abs(num) // (2 * den))              # truncates toward zero
    d16v = 16 * best + np.where((best > 0) & (best < D - 1), delta, 0)
    d16 = np.full((H, W), -16, dtype=np.int64)
    d16[:, D:] = np.where(invalid, -16, d16v)
    cost2 = np.full((H, W), INF, dtype=np.int64)
    disp2 = np.full((H, W), -1, dtype=np.int64)
    rows = np.arange(H)
    for xv in range(W1 - 1, -1, -1):                               # x from W - 1 down to D
        x2 = xv + D - best[:, xv]
        upd = ~invalid[:, xv] & (cost2[rows, x2] > minS[:, xv])
        cost2[rows[upd], x2[upd]] = minS[upd, xv]
        disp2[rows[upd], x2[upd]] = best[upd, xv]
    return d16, disp2


def lr_check(d16, disp2, max_diff):
    H, W = d16.shape
    x = np.arange(W)[None, :]
    out = d16.copy()

    def mismatch(k):
        i = x - k
        inside = (i >= 0) & (i < W)
        v = np.where(inside, np.take_along_axis(disp2, np.clip(i, 0, W - 1), axis=1), -1)
        return (v >= 0) & (np.abs(v - k) > max_diff)
    a, b = d16 >> 4, (d16 + 15) >> 4
    out[(d16 >= 0) & mismatch(a) & mismatch(b)] = -16
    return out


def median3(img):
    H, W = img.shape
    p = np.pad(img, 1, mode="edge")
    stack = np.stack([p[j:j + H, i:i + W] for j in range(3) for i in range(3)])
    return np.sort(stack, axis=0)[4]


def depth(disp16, bf=EUROC_BF):
    disp = disp16.astype(np.float64) / 16.0
    disp[disp == 0] = 1e10
    z = float(bf) / disp
    z[z < 0] = 0
    return z.astype(np.float32)


def stereo(left, right, D=64, maps=None, bf=EUROC_BF, **matcher):
    """Everything: dict(rect_l, rect_r, rgb, pc, C, S, disp16 (int16), depth (float32))."""
    q = defaults(**matcher)
    if maps is not None:
        left, right = remap_gray(left, maps[0], maps[1]), remap_gray(right, maps[2], maps[3])
    H, W = left.shape
    pcv = pc(left, right, D, q["ftzero"])
    Cv = window(pcv, q["s"])
    Sv = aggregate(Cv, q["P1"], q["P2"])
    d16, disp2 = winner(Sv, W, q["uniq"])
    disp16 = median3(lr_check(d16, disp2, q["max_diff"]))
    return dict(rect_l=left, rect_r=right, rgb=rgb(left), pc=pcv, C=Cv, S=Sv, disp16=disp16.astype(np.int16),
                depth=depth(disp16, bf))


def stereogram(H=48, W=160, seed=0):
    """The ground-truth pair of the host test: (left, right, gt [W]) -- disparity 5, 17 on columns 90..139."""
    rng = np.random.default_rng(seed)
    right = rng.integers(0, 256, (H, W + 64))[:, :W].astype(np.uint8)
    gt = np.full(W, 5)
    gt[90:140] = 17
    left = np.empty_like(right)
    for x in range(W):
        left[:, x] = right[:, x - gt[x]] if x - gt[x] >= 0 else rng.integers(0, 256, H)
    return left, right, gt


def in_plane(gt, D, W):
    """Columns x >= D whose neighbourhood [max(x - 12, D), min(x + 12, W - 1)] shares one true disparity."""
    return np.array([x >= D and len(set(gt[max(x - 12, D):min(x + 12, W - 1) + 1])) == 1 for x in range(W)])
