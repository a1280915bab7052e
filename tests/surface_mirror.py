"""The "Surface depth" specification restated on the CPU, from what the oracle already returns
(``rasterize(..., want_ambiguous=True).aux``): a per-tile walk of the lists for the median contributor and the depth variance, and
a numpy ``depth_normals``.  Not a test module: tests/test_surface_host.py ties it to the oracle, tests/test_gpu_surface.py holds the
kernels to it.

Decisions (who contributes, where a pixel stops) and the transmittances t_i are formed in the oracle's own dtype with the oracle's
own expressions (``oracle.gs_oracle._blend_tiles``); the sums O, S1, S2 of the variance are formed, in blend order, in ``sum_dtype``.
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

from monogs_amd.synthetic import make_scene

TILE = 16
INTR = dict(fx=87.0, fy=87.6, cx=52.0, cy=37.1, W=104, H=72)


def _stack():
    """Three Gaussians on the ray of the image centre, each wide enough to cover it (sigma about 40 px), opacities 0.3 / 0.4 / 0.9 at
    depths 1 / 2 / 3: at the centre pixels t = 0.7, 0.42 -- the median is the second."""
    sc = make_scene(3, INTR, seed=1)
    z = torch.tensor([1.0, 2.0, 3.0])
    pc = torch.stack([torch.zeros(3), torch.zeros(3), z], dim=1)
    return sc._replace(means3D=((pc - sc.t[None, :]) @ sc.R).contiguous(), scales=(40.0 * z / INTR["fx"])[:, None].contiguous(),
                       opacities=torch.tensor([[0.3], [0.4], [0.9]]))


def _scaled(name, f):
    sc = scene(name)
    return sc._replace(opacities=sc.opacities * f)


SCENES = dict(multi=lambda: make_scene(3000, INTR, seed=3),
              veil=lambda: _scaled("multi", 0.2),
              haze=lambda: _scaled("multi", 0.12),
              long=lambda: make_scene(12000, INTR, seed=8, mean_radius_px=12.0),
              sparse=lambda: make_scene(120, INTR, seed=6, mean_radius_px=4.0, spread=0.45),
              stack=_stack)


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def scales3(sc):
    return sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float32):
    """The oracle's forward of a scene (``want_ambiguous``); computed once per (scene, dtype), never modified."""
    from monogs_amd.synthetic import scene_settings
    from oracle import OracleSettings, rasterize
    sc = scene(name)
    return rasterize(sc.means3D, None, sc.opacities, scene_settings(sc, OracleSettings), colors_precomp=sc.colors, scales=scales3(sc),
                     rotations=sc.rotations, dtype=dtype, want_ambiguous=True)


class SurfaceMirror(NamedTuple):
    median_pos: torch.Tensor      # [H,W] int64: the 1-based list position of the median contributor, 0: none
    median_id: torch.Tensor       # [H,W] int64: its Gaussian, -1: none (or gated)
    median_depth: torch.Tensor    # [H,W]: geom["depth"] of that Gaussian, as it is; 0: none (or gated)
    depth_var: torch.Tensor       # [H,W] sum_dtype
    gated: torch.Tensor           # [H,W] bool: a gate cleared the median
    opacity_gate: torch.Tensor    # [H,W] bool: 1 - final_T < min_opacity
    z1: torch.Tensor              # [H,W] sum_dtype: the first contributor's depth (0: none)
    O: torch.Tensor               # [H,W] sum_dtype
    S1: torch.Tensor
    S2: torch.Tensor
    before_median: torch.Tensor   # [P] int64: per Gaussian, the pixels that take it with t_i > 0.5


def surface_mirror(aux, H, W, sum_dtype=torch.float64, min_opacity=0.0, max_std=0.0) -> SurfaceMirror:
    geom, point_list, ranges = aux["geom"], aux["point_list"], aux["ranges"]
    dt = geom["depth"].dtype
    gx, gy = geom["grid"]
    P = geom["depth"].shape[0]
    HP, WP = gy * TILE, gx * TILE
    pos = torch.zeros(HP, WP, dtype=torch.int64)
    mid = torch.full((HP, WP), -1, dtype=torch.int64)
    mz = torch.zeros(HP, WP, dtype=dt)
    planes = {k: torch.zeros(HP, WP, dtype=sum_dtype) for k in ("var", "z1", "O", "S1", "S2")}
    before = torch.zeros(P, dtype=torch.int64)
    lx, ly = torch.arange(TILE).repeat(TILE), torch.arange(TILE).repeat_interleave(TILE)
    for t in range(gx * gy):
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        if e <= s:
            continue
        ids = point_list[s:e]
        pxi, pyi = (t % gx) * TILE + lx, (t // gx) * TILE + ly
        inside = (pxi < W) & (pyi < H)
        xy, con, op, z = geom["xy"][ids], geom["conic"][ids], geom["opacity"][ids], geom["depth"][ids]
        dx, dy = xy[None, :, 0] - pxi.to(dt)[:, None], xy[None, :, 1] - pyi.to(dt)[:, None]                  # [256, n]
        power = -0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
        alpha = torch.clamp_max(op[None, :] * torch.exp(power), 0.99)
        skip = (power > 0) | (alpha < 1.0 / 255.0) | (~inside[:, None])
        a_eff = torch.where(skip, torch.zeros_like(alpha), alpha)
        one_m = 1.0 - a_eff
        T_incl = torch.cumprod(one_m, dim=1)
        T_before = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)
        t_i = T_before * one_m
        stopped = torch.cumsum(((~skip) & (t_i < 0.0001)).to(torch.int32), dim=1) > 0
        valid = (~skip) & (~stopped)
        idx1 = torch.arange(1, ids.shape[0] + 1)[None, :].expand_as(valid)
        n_contrib = torch.where(valid, idx1, torch.zeros_like(idx1)).amax(dim=1)
        at = valid & (t_i <= 0.5)
        has = at.any(dim=1)
        first_at = at.to(torch.int32).argmax(dim=1)                  # the first True (0 where there is none)
        before.index_add_(0, ids, (valid & (t_i > 0.5)).sum(dim=0))
        any_valid = valid.any(dim=1)
        z1 = torch.where(any_valid, z[valid.to(torch.int32).argmax(dim=1)], torch.zeros_like(z[:1])).to(sum_dtype)
        w = torch.where(valid, a_eff * T_before, torch.zeros_like(a_eff)).to(sum_dtype)
        d = z.to(sum_dtype)[None, :] - z1[:, None]
        O, S1, S2 = (torch.cumsum(v, dim=1)[:, -1] for v in (w, w * d, w * d * d))      # in blend order
        safe = torch.where(O > 0, O, torch.ones_like(O))
        var = torch.where(O > 0, torch.clamp_min(S2 / safe - (S1 / safe) ** 2, 0.0), torch.zeros_like(O))
        ys, xs = pyi, pxi
        assert torch.equal(n_contrib[inside], aux["n_contrib"][0][ys[inside], xs[inside]])      # the walk is the oracle's
        pos[ys, xs] = torch.where(has, first_at + 1, torch.zeros_like(first_at))
        mid[ys, xs] = torch.where(has, ids[first_at], torch.full_like(first_at, -1))
        mz[ys, xs] = torch.where(has, z[first_at], torch.zeros_like(z[:1]))
        for k, v in (("var", var), ("z1", z1), ("O", O), ("S1", S1), ("S2", S2)):
            planes[k][ys, xs] = v
    crop = lambda a: a[:H, :W].contiguous()  # noqa: E731
    pos, mid, mz = crop(pos), crop(mid), crop(mz)
    planes = {k: crop(v) for k, v in planes.items()}
    final_T = aux["final_T"][0]
    opacity_gate = (1.0 - final_T) < torch.tensor(min_opacity, dtype=final_T.dtype)
    gated = opacity_gate.clone()
    if max_std > 0:
        max_var = torch.tensor(max_std, dtype=torch.float32) ** 2              # float32, as the library forms it
        gated |= planes["var"] > max_var.to(sum_dtype)
    mid = torch.where(gated, torch.full_like(mid, -1), mid)
    mz = torch.where(gated, torch.zeros_like(mz), mz)
    return SurfaceMirror(pos, mid, mz, planes["var"], gated, opacity_gate, planes["z1"], planes["O"], planes["S1"], planes["S2"], before)


def depth_normals(depth, fx, fy, cx, cy, max_jump=0.0, dtype=np.float64):
    """[3,H,W]: the specification's normals of the depth image [H,W] with every operation in ``dtype``, in the order written there."""
    f = dtype
    d = np.asarray(depth).astype(f)
    H, W = d.shape
    fx, fy, cx, cy, mj = f(fx), f(fy), f(cx), f(cy), f(max_jump)
    xs, ys = np.meshgrid(np.arange(W).astype(f), np.arange(H).astype(f))
    with np.errstate(all="ignore"):
        P = np.stack([d * ((xs + f(0.5) - cx) / fx), d * ((ys + f(0.5) - cy) / fy), d])
        c, l, r, u, dn = (np.s_[:, 1:-1, 1:-1], np.s_[:, 1:-1, :-2], np.s_[:, 1:-1, 2:], np.s_[:, :-2, 1:-1], np.s_[:, 2:, 1:-1])
        a, b = P[r] - P[l], P[dn] - P[u]
        n = np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        length = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        ok = (length > 0) & np.isfinite(length)
        for s in (c, l, r, u, dn):
            ok &= d[s[1:]] > 0
            if max_jump > 0:
                ok &= ~(np.abs(d[s[1:]] - d[c[1:]]) > mj)
        n = n / np.where(ok, length, f(1))
        Pc = P[c]
        flip = n[0] * Pc[0] + n[1] * Pc[1] + n[2] * Pc[2] > 0
        n = np.where(flip, -n, n)
    out = np.zeros((3, H, W), dtype=f)
    out[:, 1:-1, 1:-1] = np.where(ok, n, f(0))
    return out
