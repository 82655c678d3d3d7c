"""CPU checker of mh_body_poses_vjp_* and mh_jacobian_transpose_*: the dense route, sum_k J_k^T (n_k; f_k) with the Jacobians and poses of
tests/kinematics_check.py (numpy; small cases only).  Deliberately not the kernel's inward accumulation of wrenches: the matrices are
formed and contracted, one configuration and one target at a time.  tests/test_kinematics_vjp_cpu.py pins this file by facts it is not
built from."""
import numpy as np

import kinematics_check as kc


def cotangent_wrench(pose, g):
    """(n; f) in the frame at `pose` (12 numbers) that the cotangent `g` of those 12 numbers stands for: M = R^T G_R,
    n = (M32 - M23, M13 - M31, M21 - M12), f = R^T g_p."""
    pose, g = np.asarray(pose, dtype=float).reshape(12), np.asarray(g, dtype=float).reshape(12)
    R = pose[:9].reshape(3, 3)
    M = R.T @ g[:9].reshape(3, 3)
    return np.concatenate([[M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]], R.T @ g[9:]])


def jacobian_transpose(m: kc.KinModel, q, wrench, targets, bases=None, poses=None):
    """[B, nv]: what mh_jacobian_transpose_* returns in AoS for wrench [B, K, 6]."""
    q = np.asarray(q, dtype=float)
    K = len(targets)
    w = np.asarray(wrench, dtype=float).reshape(q.shape[0], K, 6)
    J, _ = kc.geometric_jacobian(m, q, targets, bases, poses)
    out = np.zeros((q.shape[0], m.nv))
    for r in range(q.shape[0]):
        for k in range(K):
            out[r] += J[r, 6 * k:6 * k + 6].T @ w[r, k]
    return out


def body_poses_vjp(m: kc.KinModel, q, g_pose, targets=None, poses=None):
    """[B, nv]: what mh_body_poses_vjp_* returns in AoS for g_pose [B, K, 12] (targets=None: every body-fixed frame, K = n_joints)."""
    q = np.asarray(q, dtype=float)
    targets = list(range(m.n)) if targets is None else [int(t) for t in targets]
    K = len(targets)
    g = np.asarray(g_pose, dtype=float).reshape(q.shape[0], K, 12)
    P = kc.body_poses(m, q, targets, poses)
    w = np.array([[cotangent_wrench(P[r, k], g[r, k]) for k in range(K)] for r in range(q.shape[0])]).reshape(q.shape[0], K, 6)
    return jacobian_transpose(m, q, w, targets, None, poses)
