"""CPU checker of mh_aba_constrained_* and mh_constraint_impulse_*: the dense KKT system of every configuration, one at a time (numpy; small
cases only).

    [ H   -J_c^T ] [ qdd    ]   [ tau - h   ]              [ H   -J_c^T ] [ qd+    ]   [ H qd  ]
    [ J_c  eps I ] [ lambda ] = [ a_des - c ]              [ J_c  eps I ] [ Lambda ] = [ v_des ]

H from OracleModel.crba, h = OracleModel.rnea at qdd = 0 (gravity or root acceleration, velocity terms, minus the external wrenches), J and
c = Jdot qd from kinematics_check.geometric_jacobian with every base at the root.  J_c / c are the rows whose bit is set in target_rows[k]
and in active[r, k].  Nothing here walks the articulated-body recursion the device uses: tests/test_constrained_dynamics_cpu.py holds this
file against OracleModel.aba."""
import numpy as np

import kinematics_check as kc

POINT, WELD = 0b111000, 0b111111  # linear rows only; all six


def selected_rows(rows, active_r=None):
    """Indices into the stacked 6 K rows that take part: bit i of rows[k] (and of active_r[k]) set."""
    out = []
    for k, rk in enumerate(rows):
        ak = 0x3F if active_r is None else int(active_r[k])
        out += [6 * k + i for i in range(6) if (int(rk) >> i) & 1 and (ak >> i) & 1]
    return np.array(out, dtype=int)


def wrenches_on_bodies(desc, targets, poses, lam, f_ext=None):
    """f_ext + sum_k X_k^T lambda_k: [B, n_joints, 6] in the body-fixed frames (X_k: body -> target motion transform of pose k)."""
    B, K = lam.shape[0], len(targets)
    poses = np.tile(kc.IDENTITY12, (K, 1)) if poses is None else np.asarray(poses, dtype=float).reshape(K, 12)
    f = np.zeros((B, desc.n_joints, 6)) if f_ext is None else np.array(f_ext, dtype=float).reshape(B, desc.n_joints, 6).copy()
    for k, t in enumerate(targets):
        f[:, int(t)] += lam[:, k] @ kc.motion_into_frame(poses[k])
    return f


def _solve(H, Jc, eps, top, bottom):
    nv, m = H.shape[0], Jc.shape[0]
    KKT = np.zeros((nv + m, nv + m))
    KKT[:nv, :nv], KKT[:nv, nv:], KKT[nv:, :nv] = H, -Jc.T, Jc
    KKT[nv:, nv:] = eps * np.eye(m)
    x = np.linalg.solve(KKT, np.concatenate([top, bottom]))
    return x[:nv], x[nv:], float(np.linalg.cond(KKT, np.inf))


def _terms(om, desc, q, qd, targets, poses):
    """(H, J, c): c = Jdot qd, or None without qd"""
    m = kc.KinModel(desc)
    J, c = kc.geometric_jacobian(m, q, targets, None, poses, qd)
    return om.crba(q), J, None if c is None else c.reshape(q.shape[0], -1)


def aba_constrained(om, desc, q, qd, tau, targets, rows, poses=None, active=None, a_des=None, compliance=0.0, gravity=(0.0, 0.0, -9.81),
                    f_ext=None):
    """dict(qdd [B, nv], lam [B, K, 6], cond_kkt [B], cond_H [B], H, J, c, h): what mh_aba_constrained_* returns in AoS, with the
    conditioning of the matrix solved.  gravity: 3 entries, or 6 (a root acceleration), as OracleModel takes it."""
    q, qd, tau = (np.asarray(x, dtype=float) for x in (q, qd, tau))
    B, K = q.shape[0], len(targets)
    H, J, c = _terms(om, desc, q, qd, targets, poses)
    h = om.rnea(q, qd, np.zeros_like(qd), gravity, f_ext)
    a_des = np.zeros((B, 6 * K)) if a_des is None else np.asarray(a_des, dtype=float).reshape(B, 6 * K)
    qdd, lam, ck = np.zeros((B, desc.nv)), np.zeros((B, 6 * K)), np.zeros(B)
    for r in range(B):
        s = selected_rows(rows, None if active is None else active[r])
        qdd[r], lam[r, s], ck[r] = _solve(H[r], J[r][s], compliance, tau[r] - h[r], a_des[r, s] - c[r, s])
    return dict(qdd=qdd, lam=lam.reshape(B, K, 6), cond_kkt=ck, cond_H=np.array([np.linalg.cond(H[r], np.inf) for r in range(B)]), H=H, J=J,
                c=c, h=h)


def constraint_impulse(om, desc, q, qd, targets, rows, poses=None, active=None, v_des=None, compliance=0.0):
    """dict(qd_next, impulse [B, K, 6], cond_kkt, cond_H, H, J): what mh_constraint_impulse_* returns in AoS."""
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    B, K = q.shape[0], len(targets)
    H, J, _ = _terms(om, desc, q, None, targets, poses)
    v_des = np.zeros((B, 6 * K)) if v_des is None else np.asarray(v_des, dtype=float).reshape(B, 6 * K)
    out, imp, ck = np.zeros((B, desc.nv)), np.zeros((B, 6 * K)), np.zeros(B)
    for r in range(B):
        s = selected_rows(rows, None if active is None else active[r])
        out[r], imp[r, s], ck[r] = _solve(H[r], J[r][s], compliance, H[r] @ qd[r], v_des[r, s])
    return dict(qd_next=out, impulse=imp.reshape(B, K, 6), cond_kkt=ck, cond_H=np.array([np.linalg.cond(H[r], np.inf) for r in range(B)]), H=H,
                J=J)


def constraint_residual(R, rows, active, motion, lam, des, compliance):
    """|J_c motion + c + eps lam - des|_inf per configuration through the checker's J and c (R: a result dict; c absent: the impulse)."""
    B = motion.shape[0]
    lam, des = lam.reshape(B, -1), (np.zeros_like(lam.reshape(B, -1)) if des is None else np.asarray(des, dtype=float).reshape(B, -1))
    full = np.einsum("bij,bj->bi", R["J"], motion) + (R["c"] if "c" in R else 0.0) + compliance * lam - des
    out = np.zeros(B)
    for r in range(B):
        s = selected_rows(rows, None if active is None else active[r])
        out[r] = np.abs(full[r, s]).max() if len(s) else 0.0
    return out
