"""CPU checker of mh_contact_impulse_between_*: tests/contact_dynamics_check.py with the Jacobian of every contact taken relative to its own
base body.  Per configuration

    minimise 1/2 lam^T (S + eps I) lam + lam^T b   subject to  n_k.lam_k >= 0, |lam_k - (n_k.lam_k) n_k| <= mu_k n_k.lam_k,
    b_k = u_k - v_k n_k,   qd_next = qd + H^-1 J_l^T lam,

J_l the linear rows of kinematics_check.geometric_jacobian(m, q, targets, bases, poses): the motion of target frame k relative to the
successor body of joint bases[k] (-1: the root body), in the target frame.  S = J_l H^-1 J_l^T with its lower triangle mirrored, u = J_l qd,
n_k the normal brought from the root body frame into the target frame by the TARGET body's pose.  The sweeps are
contact_dynamics_check.sweeps, imported and not restated; cond_kkt / cond_H those of relative_constraints_check.constraint_impulse with
POINT rows, the same bases and the call's compliance.  Nothing here walks the articulated-body recursion the device uses.
tests/test_contact_between_cpu.py pins this file by facts not of its own making."""
import numpy as np

import contact_dynamics_check as cd
import kinematics_check as kc
import relative_constraints_check as rc


def terms(om, desc, q, qd, targets, bases, poses=None, normals=None, v_normal=None):
    """dict(S, b, n, J, Jl, H, norm): the quadratic form, its linear term, the normals in the target frames, the relative Jacobians and
    the mass matrix -- formed as contact_dynamics_check.terms forms them, with `bases` handed to the Jacobian"""
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    B, K = q.shape[0], len(targets)
    m = kc.KinModel(desc)
    J, _ = kc.geometric_jacobian(m, q, targets, bases, poses)
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


def solve_terms(T, qd, mu, active=None, compliance=0.0, iterations=50, init=None, history=None, precision=None, Jl_out=None):
    """dict(qd_next, impulse, residual, S, b): the sweeps on the terms T and the velocity update through Jl_out (None: T's own Jl).
    contact_impulse_between is this on terms(...); the tests hand in terms with one planted fault."""
    qd = np.asarray(qd, dtype=float)
    B, K = T["n"].shape[:2]
    mu = np.asarray(mu, dtype=float).reshape(K)
    S, b = T["S"], T["b"]
    if precision is not None:
        S, b = S.astype(precision).astype(np.float64), b.astype(precision).astype(np.float64)
    act = cd._active(active, B, K)
    lam0 = None if init is None else np.asarray(init, dtype=float).reshape(B, K, 6)[:, :, 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        lam, res = cd.sweeps(S, b, T["n"], mu, act, compliance, iterations, lam0, history)
        trace = np.stack([S[:, 3 * k, 3 * k] + S[:, 3 * k + 1, 3 * k + 1] + S[:, 3 * k + 2, 3 * k + 2] + compliance for k in range(K)], axis=1)
    ok = lambda x: np.isfinite(x) & (x > 0)
    bad = (act & ~(ok(trace) & ok(T["norm"]))).any(axis=1) | ~np.isfinite(lam).all(axis=(1, 2))
    lam[bad], res[bad] = np.nan, np.nan
    impulse = np.zeros((B, K, 6))
    impulse[:, :, 3:] = lam
    impulse[bad] = np.nan
    Jl = T["Jl"] if Jl_out is None else Jl_out
    qd_next = qd + np.linalg.solve(T["H"], np.einsum("bji,bj->bi", Jl, lam.reshape(B, -1))[:, :, None])[:, :, 0]
    return dict(qd_next=qd_next, impulse=impulse, residual=res, S=S, b=b)


def contact_impulse_between(om, desc, q, qd, targets, bases, mu, poses=None, normals=None, active=None, v_normal=None, compliance=0.0, iterations=50,
                            init=None, history=None, precision=None):
    """dict(qd_next [B, nv], impulse [B, K, 6], residual [B], S, b, n, J, Jl, H, cond_H, cond_kkt): what mh_contact_impulse_between_* returns in
    AoS, with the terms of the problem and the conditioning of the stick system.  bases=None: every base the root.  The NaN rule and
    `precision` are those of contact_dynamics_check.contact_impulse."""
    T = terms(om, desc, q, qd, targets, bases, poses, normals, v_normal)
    R = solve_terms(T, qd, mu, active, compliance, iterations, init, history, precision)
    K = len(targets)
    stick = rc.constraint_impulse(om, desc, q, qd, targets, bases, [rc.POINT] * K, poses, None, None, compliance)
    R.update(n=T["n"], J=T["J"], Jl=T["Jl"], H=T["H"], cond_H=stick["cond_H"], cond_kkt=stick["cond_kkt"])
    return R
