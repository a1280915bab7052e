"""Plain-PyTorch statement of what csrc/kfwindow.hip and monogs_amd/keyframe_window.py compute (test infrastructure, CPU).

Written from the definitions in include/monogs_raster.h, with the general 4x4 inverse (``torch.linalg.inv``) where the kernel
uses the closed form of a rigid one, in float32 or float64:

* ``lower_median``: torch's lower median of ``values[(values > lo) & (mask != 0)]`` and the element count;
* ``overlap_counts``: {|A and B_k|, |A or B_k|, |A|, |B_k|} from bool tensors;
* ``decide``: the keyframe test and both evictions on the list ``[cur] + window``;
* ``scenarios``: the seeded windows of the decision tests.  Every scenario keeps each ratio at least 1e-4 away from its
  threshold and the two best scores at least 1e-3 (relative) apart, so that rounding differences between the closed-form
  inverse in float32 and ``linalg.inv`` in float64 cannot flip a decision (asserted in tests/test_keyframe_window_host.py).

The reference's tracker cannot be imported here (it needs the rasteriser extension and the viewer at import time), so no
fixture of its own outputs pins this file: parity unpinned.
"""
import math

import torch

DEFAULTS = dict(kf_translation=0.08, kf_min_translation=0.05, kf_overlap=0.9, kf_cutoff=0.4, n_dont_touch=2)


def lower_median(values, mask=None, lo=0.0):
    v = values.reshape(-1)
    valid = v > lo
    if mask is not None:
        valid = torch.logical_and(valid, mask.reshape(-1) != 0)
    sel = v[valid]
    if sel.numel() == 0:
        return float("nan"), 0
    return sel.median().item(), int(sel.numel())


def overlap_counts(cur, rows):
    """cur bool[P], rows: list of bool[P] -> int64[K][4]."""
    out = torch.zeros(len(rows), 4, dtype=torch.int64)
    for k, b in enumerate(rows):
        out[k, 0] = torch.logical_and(cur, b).count_nonzero()
        out[k, 1] = torch.logical_or(cur, b).count_nonzero()
        out[k, 2] = cur.count_nonzero()
        out[k, 3] = b.count_nonzero()
    return out


def _T4(R, T, dtype):
    M = torch.eye(4, dtype=dtype)
    M[:3, :3] = R.to(dtype)
    M[:3, 3] = T.to(dtype)
    return M


def _dist(Ti, Tj):
    """|| t(T_i T_j^-1) ||"""
    return torch.norm((Ti @ torch.linalg.inv(Tj))[0:3, 3])


def decide(prm, counts, median, poses, dtype=torch.float64):
    """prm: dict with K, window_size, window_full, check_overlap, kf_interval, frames_since_last_kf and the thresholds;
    counts int[K][4]; poses: [(R, T)] of the current frame and the K window keyframes, most recent first.
    Returns a dict: create_kf, removed_by_cutoff, removed_by_size (positions in [cur] + window, -1 = none), iou, distance,
    median, and ``margin`` / ``score_gap``: the smallest distance of a ratio from its threshold and the relative gap of the two
    best scores (inf where there is nothing to compare)."""
    K, ws, ndt = int(prm["K"]), int(prm["window_size"]), int(prm["n_dont_touch"])
    c = counts.to(dtype)
    med = torch.tensor(median, dtype=dtype)
    Ts = [_T4(R, T, dtype) for R, T in poses]
    margins = []

    def less(x, thr):          # x < thr, remembering how close it was
        if not math.isnan(float(x)):
            margins.append(abs(float(x) - thr))
        return bool(x < thr)

    iou = c[0, 0] / c[0, 1]
    d = _dist(Ts[0], Ts[1])
    if not prm["check_overlap"]:
        create = True
    elif K < ws:
        create = less(iou, prm["kf_overlap"])
    else:
        near = less(iou, prm["kf_overlap"])
        rel = float(d / med)
        margins.extend([abs(rel - prm["kf_min_translation"]), abs(rel - prm["kf_translation"])])
        create = (near and bool(d > prm["kf_min_translation"] * med)) or bool(d > prm["kf_translation"] * med)
    create_kf = bool(create and prm["frames_since_last_kf"] >= prm["kf_interval"])

    cutoff = prm["kf_cutoff"] if prm["window_full"] else 0.4
    cut = -1
    for i in range(ndt, K + 1):
        r = c[i - 1, 0] / torch.minimum(c[i - 1, 2], c[i - 1, 3])
        if not math.isnan(float(r)):
            margins.append(abs(float(r) - cutoff))
        if bool(r <= cutoff):
            cut = i
    alive = [i for i in range(ndt, K + 1) if i != cut]
    by_size, gap = -1, float("inf")
    if K + 1 - (1 if cut >= 0 else 0) > ws:
        scores = []
        for i in alive:
            s = torch.zeros((), dtype=dtype)
            for j in alive:
                if j != i:
                    s = s + 1.0 / (_dist(Ts[i], Ts[j]) + 1e-6)
            scores.append(float(torch.sqrt(_dist(Ts[i], Ts[0])) * s))
        best = -float("inf")
        for i, s in zip(alive, scores):
            if s > best:
                best, by_size = s, i
        top = sorted(scores, reverse=True)
        if len(top) > 1 and top[0] > 0:
            gap = (top[0] - top[1]) / top[0]
    return dict(create_kf=create_kf, removed_by_cutoff=cut, removed_by_size=by_size, iou=float(iou), distance=float(d),
                median=float(med), margin=min(margins) if margins else float("inf"), score_gap=gap)


def apply_to_list(window, frame_idx, dec):
    """add_to_window on the id list: (new list, removed ids)."""
    if not dec["create_kf"]:
        return list(window), []
    new = [frame_idx] + list(window)
    removed = [new[p] for p in (dec["removed_by_cutoff"], dec["removed_by_size"]) if p >= 0]
    return [k for k in new if k not in removed], removed


# ---- seeded windows --------------------------------------------------------------------------------------------------
def _rotation(g, angle):
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm()
    Kx = torch.zeros(3, 3, dtype=torch.float64)
    Kx[0, 1], Kx[0, 2], Kx[1, 0], Kx[1, 2], Kx[2, 0], Kx[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
    R = torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    return R.to(torch.float32)


def _make(seed, K, ws, full, check, mode, P=509):
    """One window.  mode: "none" (no cut-off candidate), "several" (three candidates where the window allows), "one",
    "empty" (the current frame and the last keyframe touch nothing: every ratio is 0/0)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: float(torch.rand((), generator=g))  # noqa: E731
    perm = torch.randperm(P, generator=g)
    n_a = 0 if mode == "empty" else 200 + int(rnd() * 60)
    cur = torch.zeros(P, dtype=torch.bool)
    cur[perm[:n_a]] = True
    inside, outside = perm[:n_a], perm[n_a:]
    movable = list(range(2, K + 1))
    low = set()
    if mode == "several":
        low = set(movable[-3:])
    elif mode == "one" and movable:
        low = {movable[int(rnd() * len(movable))]}
    rows = []
    for i in range(1, K + 1):
        n_b = 150 + int(rnd() * 100)
        if mode == "empty" and i == 1:
            n_b = 0                                 # ... nor does the last keyframe: the IoU is 0/0 as well
        if i == 1:
            r = 0.55 + 0.43 * rnd()                 # the overlap with the last keyframe: either side of kf_overlap
        else:
            r = (0.05 + 0.27 * rnd()) if i in low else (0.47 + 0.45 * rnd())
        inter = min(int(round(r * min(n_a, n_b))), n_a)
        b = torch.zeros(P, dtype=torch.bool)
        b[inside[torch.randperm(n_a, generator=g)[:inter]]] = True
        b[outside[torch.randperm(P - n_a, generator=g)[:n_b - inter]]] = True
        rows.append(b)
    poses = []
    for i in range(K + 1):
        T = (torch.rand(3, generator=g) - 0.5) * 0.9            # |T| <= 0.78: keeps the float32 distances within 1e-5
        if i == 1:                                               # the last keyframe: 0.05 .. 0.4 from the current frame
            step = torch.randn(3, generator=g)
            T = poses[0][1] + step / step.norm() * (0.05 + 0.35 * rnd())
        poses.append((_rotation(g, 0.5 * rnd()), T.to(torch.float32)))
    prm = dict(DEFAULTS, K=K, window_size=ws, window_full=int(full), check_overlap=int(check), kf_interval=1 + seed % 3,
               frames_since_last_kf=1 + (seed // 3) % 3, kf_cutoff=0.3 if full else 0.4)
    return dict(seed=seed, mode=mode, prm=prm, P=P, cur=cur, rows=rows, poses=poses, median=1.0 + 2.0 * rnd())


def _well_separated(sc):
    d = decide(sc["prm"], overlap_counts(sc["cur"], sc["rows"]), sc["median"], sc["poses"], torch.float64)
    return d["margin"] >= 2e-4 and d["score_gap"] >= 2e-3


_SCENARIOS = None


def scenarios():
    """About 40 windows: K 1..11, window sizes 8 and 10, full and not, overlap check on and off, no / one / several cut-off
    candidates, both evictions in one call (K >= window size with a candidate), K <= n_dont_touch, an empty current set."""
    global _SCENARIOS
    if _SCENARIOS is not None:
        return _SCENARIOS
    spec = []
    for K in range(1, 12):
        for n, mode in enumerate(("none", "several", "one")):
            ws = 8 if (K + n) % 2 == 0 else 10
            spec.append((K, ws, (K + n) % 3 == 0, (K + n) % 2 == 1, mode))
    spec += [(11, 8, True, True, "several"), (10, 8, False, True, "several"), (11, 10, True, False, "several"),   # both evictions
             (9, 8, True, True, "none"), (8, 8, False, True, "none"), (10, 10, True, True, "one"),
             (1, 8, False, True, "empty"), (5, 8, False, True, "empty"), (11, 8, True, True, "empty"), (9, 8, False, False, "empty")]
    out = []
    for n, (K, ws, full, check, mode) in enumerate(spec):
        for attempt in range(50):
            sc = _make(1000 * n + attempt, K, ws, full, check, mode)
            if _well_separated(sc):
                out.append(sc)
                break
        else:
            raise AssertionError(f"no well-separated window for spec {n}")
    _SCENARIOS = out
    return out
