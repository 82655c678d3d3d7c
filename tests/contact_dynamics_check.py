"""CPU checker of mh_contact_impulse_*: the projected block Gauss-Seidel sweeps of include/mecano_hip.h restated in numpy, vectorised over the
batch, on S built from kinematics_check.geometric_jacobian and OracleModel.crba -- nothing here walks the articulated-body recursion the
device uses.  Per configuration

    minimise 1/2 lam^T (S + eps I) lam + lam^T b   subject to  n_k.lam_k >= 0, |lam_k - (n_k.lam_k) n_k| <= mu_k n_k.lam_k,
    b_k = u_k - v_k n_k,   qd_next = qd + H^-1 J_l^T lam,

J_l the linear rows of the Jacobian of the K target frames (every base at the root), S = J_l H^-1 J_l^T with its lower triangle mirrored
(the device mirrors block (k, l), l < k, and the lower triangle of the diagonal blocks: the same entries), u = J_l qd, n_k the normal brought
from the root body frame into the target frame.  tests/test_contact_dynamics_cpu.py pins this file by facts not of its own making."""
import itertools

import numpy as np

import constrained_dynamics_check as cc
import kinematics_check as kc


def project(x, n, mu):
    """Euclidean projection of x [B, 3] onto the cone of normal n [B, 3] and coefficient mu: the three cases of the header, no other.
    mu > 1 is worked with a = 1 / mu (r <= mu s as a r <= s, s' = a (a s + r) / (1 + a^2), the tangential factor (a s + r) / ((1 + a^2) r)):
    nothing overflows at any finite mu, and the limit is the projection onto the half space n.x >= 0."""
    s = (n * x).sum(axis=1)
    t = x - s[:, None] * n
    r = np.sqrt((t * t).sum(axis=1))
    wide = mu > 1.0
    m = 1.0 / mu if wide else mu
    inside = m * r <= s if wide else r <= m * s
    polar = ~inside & (r <= -(m * s) if wide else m * r <= -s)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = ((m * s + r) if wide else (s + m * r)) / (1.0 + m * m)
        s1, c = (m * w, w / r) if wide else (w, m * w / r)
        y = s1[:, None] * n + c[:, None] * t
    return np.where(inside[:, None], x, np.where(polar[:, None], 0.0, y))


def _active(active, B, K):
    return np.ones((B, K), dtype=bool) if active is None else np.asarray(active).reshape(B, K) != 0


def objective(S, b, eps, lam):
    """1/2 lam^T (S + eps I) lam + lam^T b per configuration; lam [B, K, 3]"""
    x = lam.reshape(lam.shape[0], -1)
    return 0.5 * np.einsum("bi,bij,bj->b", x, S, x) + 0.5 * eps * (x * x).sum(axis=1) + (x * b).sum(axis=1)


def sweeps(S, b, n, mu, active, eps, iterations, lam0=None, history=None):
    """(lam [B, K, 3], residual [B]): lam0 projected, then `iterations` sweeps k = 0 ... K - 1 with the newest lam, closed contacts only.
    history: a list that receives the objective after the projection and after every sweep."""
    B, K = n.shape[:2]
    act = _active(active, B, K)
    lam = np.zeros((B, K, 3))
    if lam0 is not None:
        for k in range(K):
            lam[:, k] = np.where(act[:, k, None], project(np.asarray(lam0, dtype=float).reshape(B, K, 3)[:, k], n[:, k], mu[k]), 0.0)
    if history is not None:
        history.append(objective(S, b, eps, lam))
    res = np.zeros(B)
    for _ in range(iterations):
        res = np.zeros(B)
        for k in range(K):
            rows = slice(3 * k, 3 * k + 3)
            u = b[:, rows] + np.einsum("bij,bj->bi", S[:, rows, :], lam.reshape(B, -1)) + eps * lam[:, k]
            rho = 1.0 / (S[:, 3 * k, 3 * k] + S[:, 3 * k + 1, 3 * k + 1] + S[:, 3 * k + 2, 3 * k + 2] + eps)
            new = np.where(act[:, k, None], project(lam[:, k] - rho[:, None] * u, n[:, k], mu[k]), 0.0)
            res = np.maximum(res, np.abs(new - lam[:, k]).max(axis=1))
            lam[:, k] = new
        if history is not None:
            history.append(objective(S, b, eps, lam))
    return lam, res


def terms(om, desc, q, qd, targets, poses=None, normals=None, v_normal=None):
    """dict(S, b, n, J, Jl, H): the quadratic form, its linear term, the normals in the target frames, the Jacobians and the mass matrix"""
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    B, K = q.shape[0], len(targets)
    m = kc.KinModel(desc)
    J, _ = kc.geometric_jacobian(m, q, targets, None, poses)
    H = om.crba(q)
    lin = np.array([6 * k + 3 + i for k in range(K) for i in range(3)])
    Jl = J[:, lin, :]
    W = np.einsum("bij,bkj->bik", Jl, np.linalg.solve(H, Jl.transpose(0, 2, 1)).transpose(0, 2, 1))
    S = np.tril(W) + np.tril(W, -1).transpose(0, 2, 1)
    nh = np.tile(np.array([0.0, 0.0, 1.0]), (B, K, 1)) if normals is None else np.asarray(normals, dtype=float).reshape(B, K, 3)
    norm = np.sqrt((nh * nh).sum(axis=2))
    with np.errstate(divide="ignore", invalid="ignore"):
        nh = nh / norm[:, :, None]
    R = kc.body_poses(m, q, targets, poses)[:, :, :9].reshape(B, K, 3, 3)  # x_root = R x_target + p
    n = np.einsum("bkji,bkj->bki", R, nh)
    v = np.zeros((B, K)) if v_normal is None else np.asarray(v_normal, dtype=float).reshape(B, K)
    b = np.einsum("bij,bj->bi", Jl, qd) - (v[:, :, None] * n).reshape(B, -1)
    return dict(S=S, b=b, n=n, J=J, Jl=Jl, H=H, norm=norm)


def contact_impulse(om, desc, q, qd, targets, mu, poses=None, normals=None, active=None, v_normal=None, compliance=0.0, iterations=50, init=None,
                    history=None, precision=None):
    """dict(qd_next [B, nv], impulse [B, K, 6], residual [B], S, b, n, J, H, cond_H, cond_kkt): what mh_contact_impulse_* returns in AoS, with
    the terms of the problem and the conditioning of the stick system (all K contacts as POINT rows of cc.constraint_impulse with the
    call's compliance).  A configuration whose trace S_kk + eps or normal length is not positive and finite for a closed contact, or whose
    impulses after the last sweep are not finite, is NaN throughout.  precision: round S and b to this dtype before the sweeps (how far the call's precision can move the iterates)."""
    qd = np.asarray(qd, dtype=float)
    B, K = qd.shape[0], len(targets)
    mu = np.asarray(mu, dtype=float).reshape(K)
    T = terms(om, desc, q, qd, targets, poses, normals, v_normal)
    S, b = T["S"], T["b"]
    if precision is not None:
        S, b = S.astype(precision).astype(np.float64), b.astype(precision).astype(np.float64)
    act = _active(active, B, K)
    lam0 = None if init is None else np.asarray(init, dtype=float).reshape(B, K, 6)[:, :, 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        lam, res = sweeps(S, b, T["n"], mu, act, compliance, iterations, lam0, history)
        trace = np.stack([S[:, 3 * k, 3 * k] + S[:, 3 * k + 1, 3 * k + 1] + S[:, 3 * k + 2, 3 * k + 2] + compliance for k in range(K)], axis=1)
    ok = lambda x: np.isfinite(x) & (x > 0)
    bad = (act & ~(ok(trace) & ok(T["norm"]))).any(axis=1) | ~np.isfinite(lam).all(axis=(1, 2))
    lam[bad], res[bad] = np.nan, np.nan
    impulse = np.zeros((B, K, 6))
    impulse[:, :, 3:] = lam
    impulse[bad] = np.nan
    qd_next = qd + np.linalg.solve(T["H"], np.einsum("bji,bj->bi", T["Jl"], lam.reshape(B, -1))[:, :, None])[:, :, 0]
    stick = cc.constraint_impulse(om, desc, q, qd, targets, [cc.POINT] * K, poses, None, None, compliance)
    return dict(qd_next=qd_next, impulse=impulse, residual=res, S=S, b=b, n=T["n"], J=T["J"], H=T["H"], cond_H=stick["cond_H"], cond_kkt=stick["cond_kkt"])


def natural_residual(S, b, n, mu, active, eps, lam):
    """max_k |lam_k - Pi_k(lam_k - u_k)|_inf per configuration, u = b + (S + eps I) lam: zero exactly at the minimiser.  lam [B, K, 3]"""
    B, K = n.shape[:2]
    act = _active(active, B, K)
    u = (b + np.einsum("bij,bj->bi", S, lam.reshape(B, -1)) + eps * lam.reshape(B, -1)).reshape(B, K, 3)
    out = np.zeros(B)
    for k in range(K):
        d = np.abs(lam[:, k] - project(lam[:, k] - u[:, k], n[:, k], mu[k])).max(axis=1)
        out = np.maximum(out, np.where(act[:, k], d, np.abs(lam[:, k]).max(axis=1)))
    return out


def frictionless_exact(S, b, n, active, eps):
    """The mu = 0 solution lam [B, K, 3] = x_k n_k by enumeration: 0 <= x _|_ A x + c >= 0 with A = N S N^T + eps I over the 2^K sets of
    pressing contacts (A is positive definite: one set satisfies both signs; rounding is settled by the least violation)."""
    B, K = n.shape[:2]
    act = _active(active, B, K)
    lam = np.zeros((B, K, 3))
    for r in range(B):
        N = np.zeros((K, 3 * K))
        for k in range(K):
            N[k, 3 * k:3 * k + 3] = n[r, k]
        A, c = N @ S[r] @ N.T + eps * np.eye(K), N @ b[r]
        closed = [k for k in range(K) if act[r, k]]
        best, best_x = np.inf, np.zeros(K)
        for size in range(len(closed) + 1):
            for s in itertools.combinations(closed, size):
                s = list(s)
                x = np.zeros(K)
                if s:
                    x[s] = np.linalg.solve(A[np.ix_(s, s)], -c[s])
                w = A @ x + c
                rest = [k for k in closed if k not in s]
                viol = max([0.0] + [-x[k] for k in s] + [-w[k] for k in rest])
                if viol < best:
                    best, best_x = viol, x
        lam[r] = best_x[:, None] * n[r]
    return lam
