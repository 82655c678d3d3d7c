"""CPU checker of mh_aba_constrained_between_* and mh_constraint_impulse_between_*: the dense KKT system of
tests/constrained_dynamics_check.py with the Jacobian of every target frame taken relative to its own base body,

    [ H   -J_c^T ] [ qdd    ]   [ tau - h   ]              [ H   -J_c^T ] [ qd+    ]   [ H qd  ]
    [ J_c  eps I ] [ lambda ] = [ a_des - c ]              [ J_c  eps I ] [ Lambda ] = [ v_des ]

J and c = Jdot qd from kinematics_check.geometric_jacobian(m, q, targets, bases, poses, qd): the motion of target frame k relative to the
successor body of joint bases[k] (-1: the root body), expressed in the target frame.  lambda_k is the wrench on the target body at and in
the target frame; the base body receives the opposite wrench at the same point (`wrenches_on_bodies`).  Nothing here walks the
articulated-body recursion the device uses: tests/test_relative_constraints_cpu.py holds this file against OracleModel.aba, against the
rooted checker and against a parallelogram linkage with a closed-form answer."""
import numpy as np

import constrained_dynamics_check as cc
import kinematics_check as kc

POINT, WELD = cc.POINT, cc.WELD
selected_rows = cc.selected_rows
constraint_residual = cc.constraint_residual


def wrenches_on_bodies(m, q, targets, bases, poses, lam, f_ext=None):
    """f_ext + sum_k (X_k^T lambda_k on the target body - Z_k^T lambda_k on the base body): [B, n_joints, 6] in the body-fixed frames.
    X_k: body -> target motion transform of pose k; Z_k: the motion transform from the base's body-fixed frame to the target frame at
    q.  A root base receives nothing."""
    q = np.asarray(q, dtype=float)
    B, K = lam.shape[0], len(targets)
    bases = [-1] * K if bases is None else [int(b) for b in bases]
    poses = np.tile(kc.IDENTITY12, (K, 1)) if poses is None else np.asarray(poses, dtype=float).reshape(K, 12)
    lam = np.asarray(lam, dtype=float).reshape(B, K, 6)
    f = np.zeros((B, m.n, 6)) if f_ext is None else np.array(f_ext, dtype=float).reshape(B, m.n, 6).copy()
    for k, t in enumerate(targets):
        f[:, int(t)] += lam[:, k] @ kc.motion_into_frame(poses[k])
    for r in range(B):
        T0 = kc.joint_frames(m, q[r])
        for k, (t, b) in enumerate(zip(targets, bases)):
            if b >= 0:
                Z = kc.Ad(kc.T_inv(kc.frame_of(m, T0, int(t), poses[k])) @ kc.frame_of(m, T0, b))
                f[r, b] -= lam[r, k] @ Z
    return f


def _terms(om, desc, q, qd, targets, bases, poses):
    """(H, J, c): c = Jdot qd, or None without qd"""
    J, c = kc.geometric_jacobian(kc.KinModel(desc), q, targets, bases, poses, qd)
    return om.crba(q), J, None if c is None else c.reshape(q.shape[0], -1)


def aba_constrained(om, desc, q, qd, tau, targets, bases, rows, poses=None, active=None, a_des=None, compliance=0.0,
                    gravity=(0.0, 0.0, -9.81), f_ext=None):
    """dict(qdd [B, nv], lam [B, K, 6], cond_kkt [B], cond_H [B], H, J, c, h): what mh_aba_constrained_between_* returns in AoS."""
    q, qd, tau = (np.asarray(x, dtype=float) for x in (q, qd, tau))
    B, K = q.shape[0], len(targets)
    H, J, c = _terms(om, desc, q, qd, targets, bases, poses)
    h = om.rnea(q, qd, np.zeros_like(qd), gravity, f_ext)
    a_des = np.zeros((B, 6 * K)) if a_des is None else np.asarray(a_des, dtype=float).reshape(B, 6 * K)
    qdd, lam, ck = np.zeros((B, desc.nv)), np.zeros((B, 6 * K)), np.zeros(B)
    for r in range(B):
        s = selected_rows(rows, None if active is None else active[r])
        qdd[r], lam[r, s], ck[r] = cc._solve(H[r], J[r][s], compliance, tau[r] - h[r], a_des[r, s] - c[r, s])
    return dict(qdd=qdd, lam=lam.reshape(B, K, 6), cond_kkt=ck, cond_H=np.array([np.linalg.cond(H[r], np.inf) for r in range(B)]), H=H, J=J,
                c=c, h=h)


def constraint_impulse(om, desc, q, qd, targets, bases, rows, poses=None, active=None, v_des=None, compliance=0.0, terms=None):
    """dict(qd_next, impulse [B, K, 6], cond_kkt, cond_H, H, J): what mh_constraint_impulse_between_* returns in AoS.  terms: a result
    of `aba_constrained` for the same q, targets, bases and poses, whose H and J are taken instead of being formed again."""
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    B, K = q.shape[0], len(targets)
    H, J = (terms["H"], terms["J"]) if terms is not None else _terms(om, desc, q, None, targets, bases, poses)[:2]
    v_des = np.zeros((B, 6 * K)) if v_des is None else np.asarray(v_des, dtype=float).reshape(B, 6 * K)
    out, imp, ck = np.zeros((B, desc.nv)), np.zeros((B, 6 * K)), np.zeros(B)
    for r in range(B):
        s = selected_rows(rows, None if active is None else active[r])
        out[r], imp[r, s], ck[r] = cc._solve(H[r], J[r][s], compliance, H[r] @ qd[r], v_des[r, s])
    return dict(qd_next=out, impulse=imp.reshape(B, K, 6), cond_kkt=ck, cond_H=np.array([np.linalg.cond(H[r], np.inf) for r in range(B)]), H=H,
                J=J)
