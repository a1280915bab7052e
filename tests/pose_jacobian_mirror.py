"""Float64 references of the pose-tangent tests (tests/test_pose_jacobian_host.py, tests/test_gpu_pose_jacobian.py).

* ``oracle_jacobian``: the per-pixel Jacobian of the oracle's render with respect to tau = (rho, theta), by the double-backward
  construction: with ``out = cat(color, depth, opacity)`` and a dummy cotangent ``v``, ``g = grad(out, tau, v, create_graph=True)``
  is linear in ``v`` and column k of the Jacobian is ``grad(g[k], v)``.  It differentiates the oracle's own graph, so it respects
  the oracle's three gradient conventions (decisions constant, a clamped ratio constant, the 0.99 cap straight-through).
* ``normal_equations``: the rows of DESIGN.md section 3 ("Pose tangents") in float64, the Huber weight formed in float32.
* ``gn_step``: the damped solve (numpy) and the retraction with the oracle's ``se3_exp``.
"""
import numpy as np
import torch

from oracle import gs_oracle, rasterize

D = torch.float64


def oracle_jacobian(inp, settings, dtype=D, want_ambiguous=False):
    """``(J [6, 5, H, W], out)``: ``J[k, c]`` = d (R, G, B, depth, opacity)[c] / d tau_k in ``dtype``; ``out`` the oracle's forward
    (``out.aux["ambiguous"]`` with ``want_ambiguous``)."""
    rho = torch.zeros(3, dtype=dtype, requires_grad=True)
    theta = torch.zeros(3, dtype=dtype, requires_grad=True)
    o = rasterize(inp["means3D"], None, inp["opacities"], settings, shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"),
                  scales=inp.get("scales"), rotations=inp.get("rotations"), cov3D_precomp=inp.get("cov3D_precomp"),
                  theta=theta, rho=rho, dtype=dtype, want_ambiguous=want_ambiguous)
    out = torch.cat([o.color, o.depth, o.opacity], dim=0)
    H, W = out.shape[-2:]
    J = torch.zeros(6, 5, H, W, dtype=dtype)
    if not out.requires_grad:                    # nothing in front of the camera
        return J, o
    v = torch.zeros_like(out, requires_grad=True)
    g_rho, g_theta = torch.autograd.grad(out, [rho, theta], v, create_graph=True, allow_unused=True)
    for k in range(6):
        gk = (g_rho if k < 3 else g_theta)
        if gk is None or not gk.requires_grad:
            continue
        (col,) = torch.autograd.grad(gk[k % 3], v, retain_graph=True, allow_unused=True)
        if col is not None:
            J[k] = col
    return J, o


def huber(r64, delta):
    """(omega, rho): omega = 1 if |r| <= delta else delta / |r| with r and delta in float32; rho the Huber cost in float64."""
    r32 = r64.to(torch.float32).abs()
    d32 = torch.tensor(delta, dtype=torch.float32)
    inside = r32 <= d32
    omega = torch.where(inside, torch.ones_like(r32), d32 / r32).to(D)
    d = float(np.float32(delta))
    rho = torch.where(inside, 0.5 * r64 * r64, d * (r64.abs() - 0.5 * d))
    return omega, rho


def normal_equations(J, color, depth, opacity, gt_rgb, gt_depth, mask, grad_mask, a, b, delta_rgb, delta_depth, rgb_only=False):
    """``(H [8, 8], g [8], E, N_rgb, N_d)`` in float64 from float32 (or float64) images.  J: [6, 5, H, W] or [30, H, W]."""
    Hh, Ww = color.shape[-2:]
    J = J.reshape(6, 5, Hh, Ww).to(D)
    C, I, O = color.to(D).reshape(3, -1), gt_rgb.to(D).reshape(3, -1), opacity.reshape(-1)
    ea, eb = float(np.exp(np.float64(np.float32(a)))), float(np.float32(b))
    HW = Hh * Ww
    H, g, E = torch.zeros(8, 8, dtype=D), torch.zeros(8, dtype=D), 0.0
    m = (O > 0.99) & grad_mask.reshape(-1).bool()
    if mask is not None:
        m = m & mask.reshape(-1).bool()
    s = 0.5 / (3.0 * HW)
    for c in range(3):
        r = ea * C[c] + eb - I[c]
        jv = torch.cat([ea * J[:, c].reshape(6, -1), (ea * C[c])[None], torch.ones(1, HW, dtype=D)], dim=0)[:, m]
        omega, rho = huber(r[m], delta_rgb)
        H += s * (jv * omega) @ jv.t()
        g += s * (jv * (omega * r[m])).sum(dim=1)
        E += s * float(rho.sum())
    n_rgb, n_d = int(m.sum()), 0
    if not rgb_only:
        md = (gt_depth.reshape(-1) > 0) & (O > 0.99)
        n_d = int(md.sum())
        if n_d > 0:
            r = (depth.to(D).reshape(-1) - gt_depth.to(D).reshape(-1))[md]
            jv = J[:, 3].reshape(6, -1)[:, md]
            omega, rho = huber(r, delta_depth)
            H[:6, :6] += (jv * omega) @ jv.t() / n_d
            g[:6] += (jv * (omega * r)).sum(dim=1) / n_d
            E += float(rho.sum()) / n_d
    return H, g, E, n_rgb, n_d


def gn_step(H, g, R, T, a, b, lam, lam_abs, max_rot, max_trans, fix_exposure=False):
    """``(R, T, a, b, |tau|, ok)`` after one damped step: (H + lam diag(H) + lam_abs I) x = -g, the whole step scaled into the
    clamps, T_cw <- se3_exp([rho; theta]) T_cw.  ``ok`` False (nothing moved): the damped matrix is not positive definite."""
    n = 6 if fix_exposure else 8
    A = H[:n, :n].numpy().copy()
    A[np.diag_indices(n)] += lam * np.diag(A) + lam_abs
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return R, T, a, b, 0.0, False
    x = np.zeros(8)
    x[:n] = np.linalg.solve(A, -g[:n].numpy())
    nr, nt = np.linalg.norm(x[:3]), np.linalg.norm(x[3:6])
    sc = 1.0
    if nt > max_rot:
        sc = max_rot / nt
    if nr * sc > max_trans:
        sc = max_trans / nr
    x = x * sc
    Tm = torch.eye(4, dtype=D)
    Tm[:3, :3], Tm[:3, 3] = R.to(D), T.to(D)
    Tn = gs_oracle.se3_exp(torch.tensor(x[:6], dtype=D)) @ Tm
    return Tn[:3, :3], Tn[:3, 3], a + x[6], b + x[7], float(np.linalg.norm(x[:6])), True
