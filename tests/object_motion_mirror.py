"""TEST INFRASTRUCTURE: rigid object motion restated in float64 torch ("Object motion"): ``exp(tau^)`` composed with an
object's ``(R, t)``, the forward through it, and the gradients by autograd at ``tau = 0``.  Where this file and the closed forms of
the kernels disagree, this file is the specification (tests/test_object_motion_host.py holds the two together to 1e-12)."""
import numpy as np
import torch

F64 = torch.float64


def skew(v):
    z = torch.zeros((), dtype=v.dtype)
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


def se3_exp(tau):
    """``tau = [rho; theta]`` -> ``(R, t)`` of ``exp(tau^)``, differentiable at 0 (the series below 1e-5, as ``pose_utils`` switches)."""
    rho, th = tau[:3], tau[3:]
    K = skew(th)
    K2 = K @ K
    a = float(th.detach().norm())
    eye = torch.eye(3, dtype=tau.dtype)
    if a < 1e-5:
        return eye + K + 0.5 * K2, (eye + 0.5 * K + K2 / 6.0) @ rho
    an = th.norm()
    R = eye + (torch.sin(an) / an) * K + ((1 - torch.cos(an)) / an ** 2) * K2
    V = eye + ((1 - torch.cos(an)) / an ** 2) * K + ((an - torch.sin(an)) / an ** 3) * K2
    return R, V @ rho


def quat_exp(th):
    """The unit quaternion ``(r, x, y, z)`` of the rotation vector ``th``, differentiable at 0."""
    a = float(th.detach().norm())
    if a < 1e-5:
        n2 = (th * th).sum()
        return torch.cat([(1 - n2 / 8.0).reshape(1), th * (0.5 - n2 / 48.0)])
    an = th.norm()
    return torch.cat([torch.cos(an / 2).reshape(1), torch.sin(an / 2) * th / an])


def quat_mul(a, b):
    """Hamilton product, ``(r, x, y, z)``, broadcasting over leading dimensions."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def quat_of(R):
    """``quat(R)``: Shepperd's four branches (the largest of the trace and the diagonal decides), float64."""
    m = np.asarray(R, np.float64)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0.0:
        d = np.sqrt(tr + 1.0) * 2.0
        q = (0.25 * d, (m[2, 1] - m[1, 2]) / d, (m[0, 2] - m[2, 0]) / d, (m[1, 0] - m[0, 1]) / d)
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        d = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2.0
        q = ((m[2, 1] - m[1, 2]) / d, 0.25 * d, (m[0, 1] + m[1, 0]) / d, (m[0, 2] + m[2, 0]) / d)
    elif m[1, 1] > m[2, 2]:
        d = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2.0
        q = ((m[0, 2] - m[2, 0]) / d, (m[0, 1] + m[1, 0]) / d, 0.25 * d, (m[1, 2] + m[2, 1]) / d)
    else:
        d = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2.0
        q = ((m[1, 0] - m[0, 1]) / d, (m[0, 2] + m[2, 0]) / d, (m[1, 2] + m[2, 1]) / d, 0.25 * d)
    return torch.tensor(q, dtype=F64)


def slots(labels, slot_of_label, M):
    """[P] long: the pose slot of every Gaussian, -1: static (a table entry outside 0..M-1 counts as -1)."""
    s = torch.as_tensor(slot_of_label).long()[torch.as_tensor(labels).long()]
    return torch.where((s >= 0) & (s < M), s, torch.full_like(s, -1))


def _apply(slot, Rs, ts, qs, x, q):
    """``(R_m x + t_m, q_m (x) q)`` for the moved rows, the inputs for the others.  ``Rs [M,3,3]``, ``ts [M,3]``, ``qs [M,4]``."""
    moved = slot >= 0
    if Rs.shape[0] == 0 or not bool(moved.any()):
        return x, q
    s = slot.clamp_min(0)
    x2 = torch.where(moved[:, None], torch.einsum("pij,pj->pi", Rs[s], x) + ts[s], x)
    q2 = None if q is None else torch.where(moved[:, None], quat_mul(qs[s], q), q)
    return x2, q2


def forward(x, q, labels, slot_of_label, R, t):
    """``(x', q')`` in float64 (``q`` may be None)."""
    R, t = torch.as_tensor(R).to(F64).reshape(-1, 3, 3), torch.as_tensor(t).to(F64).reshape(-1, 3)
    M = R.shape[0]
    qs = torch.stack([quat_of(R[m]) for m in range(M)]) if M else torch.zeros(0, 4, dtype=F64)
    return _apply(slots(labels, slot_of_label, M), R, t, qs, torch.as_tensor(x).to(F64), None if q is None else torch.as_tensor(q).to(F64))


def backward(x_out, q_out, labels, slot_of_label, R, g, gq):
    """Autograd gradients of ``L = sum g . x'' + sum gq . q''`` with ``(x'', q'') = exp(tau_m^) (x', q')`` at ``tau = 0`` and
    ``(x', q') = (R_m x + t_m, quat(R_m) (x) q)``: ``(grad_tau [M,6] rho then theta, grad_x [P,3], grad_q [P,4] or None)``.  ``x_out``,
    ``q_out``: the forward's outputs (the kernels read them back, so the mirror is handed the same numbers)."""
    R = torch.as_tensor(R).to(F64).reshape(-1, 3, 3)
    M = R.shape[0]
    slot = slots(labels, slot_of_label, M)
    x_out, g = torch.as_tensor(x_out).to(F64), torch.as_tensor(g).to(F64)
    has_q = gq is not None
    q_out = torch.as_tensor(q_out).to(F64) if has_q else None
    gq = torch.as_tensor(gq).to(F64) if has_q else None
    # ---- the tangent: exp(tau^) on the outputs
    tau = torch.zeros(M, 6, dtype=F64, requires_grad=True)
    grad_tau = torch.zeros(M, 6, dtype=F64)
    if M:
        ex = [se3_exp(tau[m]) for m in range(M)]
        x2, q2 = _apply(slot, torch.stack([e[0] for e in ex]), torch.stack([e[1] for e in ex]),
                        torch.stack([quat_exp(tau[m, 3:]) for m in range(M)]), x_out, q_out)
        L = (g * x2).sum() + ((gq * q2).sum() if has_q else 0.0)
        if L.requires_grad:
            grad_tau = torch.autograd.grad(L, tau)[0]
    # ---- the inputs: through (R, t) itself (t drops out of the gradient)
    x = torch.zeros_like(x_out).requires_grad_(True)
    q = torch.zeros_like(q_out).requires_grad_(True) if has_q else None
    qs = torch.stack([quat_of(R[m]) for m in range(M)]) if M else torch.zeros(0, 4, dtype=F64)
    x1, q1 = _apply(slot, R, torch.zeros(M, 3, dtype=F64), qs, x, q)
    L = (g * x1).sum() + ((gq * q1).sum() if has_q else 0.0)
    grads = torch.autograd.grad(L, [x] + ([q] if has_q else []))
    return grad_tau, grads[0], grads[1] if has_q else None


def closed_form_tau(x_out, q_out, slot, M, g, gq):
    """The formulas the kernels implement: ``dL/drho_m = sum g_i``, ``dL/dtheta_m = sum x'_i x g_i`` and, with a rotation gradient,
    ``+ 1/2 (w gq_v - gq_w v + v x gq_v)`` for ``q' = (w, v)``.  Returns ``(grad_tau [M,6], abs_terms [M,6], counts [M])``:
    ``abs_terms`` is the sum of the absolute values of every product that enters a sum (the ``sum |term|`` of the test's bound)."""
    x_out, g = torch.as_tensor(x_out).to(F64), torch.as_tensor(g).to(F64)
    tau, absn, counts = torch.zeros(M, 6, dtype=F64), torch.zeros(M, 6, dtype=F64), torch.zeros(M, dtype=torch.long)
    cr = lambda a, b: torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],  # noqa: E731
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    cra = lambda a, b: torch.stack([(a[:, 1] * b[:, 2]).abs() + (a[:, 2] * b[:, 1]).abs(),  # noqa: E731
                                    (a[:, 2] * b[:, 0]).abs() + (a[:, 0] * b[:, 2]).abs(),
                                    (a[:, 0] * b[:, 1]).abs() + (a[:, 1] * b[:, 0]).abs()], 1)
    for m in range(M):
        sel = slot == m
        counts[m] = int(sel.sum())
        xm, gm = x_out[sel], g[sel]
        th, tha = cr(xm, gm), cra(xm, gm)
        if gq is not None:
            qm, gqm = torch.as_tensor(q_out).to(F64)[sel], torch.as_tensor(gq).to(F64)[sel]
            w, v, gw, gv = qm[:, :1], qm[:, 1:], gqm[:, :1], gqm[:, 1:]
            th = th + 0.5 * (w * gv - gw * v + cr(v, gv))
            tha = tha + 0.5 * ((w * gv).abs() + (gw * v).abs() + cra(v, gv))
        tau[m, :3], tau[m, 3:] = gm.sum(0), th.sum(0)
        absn[m, :3], absn[m, 3:] = gm.abs().sum(0), tha.sum(0)
    return tau, absn, counts


def retract(R, t, rho, theta):
    """``T <- exp([rho; theta]^) T`` in float64: ``(R', t')``."""
    dR, dt = se3_exp(torch.cat([torch.as_tensor(rho).to(F64), torch.as_tensor(theta).to(F64)]))
    R, t = torch.as_tensor(R).to(F64), torch.as_tensor(t).to(F64)
    return dR @ R, dR @ t + dt
