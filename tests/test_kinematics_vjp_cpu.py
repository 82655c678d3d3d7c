"""Pins of the CPU checker of the reverse-mode kinematics calls (tests/kinematics_vjp_check.py) by facts it is not built from -- central
differences of the poses, a closed form for tangent cotangents, the C oracle's inverse dynamics, a central difference with respect to the
raw coordinates for chart_pullback -- and the target lists the device tests share.  No GPU."""
import numpy as np
import pytest

import kinematics_check as kc
import kinematics_vjp_check as kv
from helpers import close
from oracle.cpu_oracle import OracleModel
from test_kinematics_cpu import CASES, make_case, states, targets_of


def posed_targets(case, desc, K, seed=50):
    """(targets, poses): K posed targets; with K >= 3 one body is named twice (targets_of) and the root body is among them."""
    t, _ = targets_of(case, desc, K)
    if K >= 3:
        t[-1] = t[1]
        t[2] = -1
    return t, kc.random_poses(np.random.default_rng(seed + K), K)


def cotangents(B, K, per_target, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, K, per_target))


def loss(m, q, g, t, poses):
    return float((g * kc.body_poses(m, q[None], t, poses)[0]).sum())


@pytest.mark.parametrize("case", CASES)
def test_central_differences_of_the_poses(case):
    """sum g . (pose(q (+) eps e_j) - pose(q (-) eps e_j)) / 2 eps for every DoF index j is gq[j].  eps = 1e-5, held to 12 K 1e-8: the
    1e-8 test_pose_differences_reproduce_the_jacobian holds the same difference of one entry to, times the 12 K cotangent entries of
    magnitude <= 1."""
    sys_, desc = make_case(case)
    m = kc.KinModel(desc)
    K, B, eps = 5, 2, 1.0e-5
    t, poses = posed_targets(case, desc, K)
    assert -1 in t and len(set(t)) < K
    q = states(sys_, desc, B)[0]
    g = cotangents(B, K, 12, 60)
    gq = kv.body_poses_vjp(m, q, g, t, poses)
    worst = 0.0
    for r in range(B):
        for j in range(desc.nv):
            e = np.zeros(desc.nv)
            e[j] = eps
            d = (loss(m, kc.configuration_add(m, q[r], e), g[r], t, poses) - loss(m, kc.configuration_add(m, q[r], -e), g[r], t, poses)) / (2 * eps)
            worst = max(worst, abs(d - gq[r, j]))
    print(f"{case}: worst |difference quotient - gq| = {worst:.3e}")
    assert worst <= 12 * K * 1.0e-8
    assert np.abs(gq).max() > 0.1


@pytest.mark.parametrize("case", CASES)
def test_central_differences_of_every_body(case):
    """The all-bodies form: the cotangent of every body-fixed frame, in joint order; the same bound with K = n_joints."""
    sys_, desc = make_case(case)
    m = kc.KinModel(desc)
    K, eps = desc.n_joints, 1.0e-5
    q = states(sys_, desc, 1)[0]
    g = cotangents(1, K, 12, 61)
    gq = kv.body_poses_vjp(m, q, g)
    worst = 0.0
    for j in range(desc.nv):
        e = np.zeros(desc.nv)
        e[j] = eps
        d = (loss(m, kc.configuration_add(m, q[0], e), g[0], None, None) - loss(m, kc.configuration_add(m, q[0], -e), g[0], None, None)) / (2 * eps)
        worst = max(worst, abs(d - gq[0, j]))
    assert worst <= 12 * K * 1.0e-8


@pytest.mark.parametrize("case", CASES)
def test_tangent_cotangents(case):
    """G_R = R [a]x, g_p = R b is the cotangent that the wrench (2 a; b) stands for: M = [a]x, whose antisymmetric part read as a vector
    is 2 a.  The two checker routes agree on it."""
    sys_, desc = make_case(case)
    m = kc.KinModel(desc)
    K, B = 4, 2
    t, poses = posed_targets(case, desc, K)
    q = states(sys_, desc, B)[0]
    rng = np.random.default_rng(62)
    a, b = rng.uniform(-1, 1, (B, K, 3)), rng.uniform(-1, 1, (B, K, 3))
    P = kc.body_poses(m, q, t, poses)
    g = np.zeros((B, K, 12))
    for r in range(B):
        for k in range(K):
            R = P[r, k, :9].reshape(3, 3)
            ax = np.array([[0, -a[r, k, 2], a[r, k, 1]], [a[r, k, 2], 0, -a[r, k, 0]], [-a[r, k, 1], a[r, k, 0], 0]])
            g[r, k, :9], g[r, k, 9:] = (R @ ax).reshape(9), R @ b[r, k]
            assert np.abs(kv.cotangent_wrench(P[r, k], g[r, k]) - np.concatenate([2 * a[r, k], b[r, k]])).max() <= 1e-14
    close(kv.body_poses_vjp(m, q, g, t, poses), kv.jacobian_transpose(m, q, np.concatenate([2 * a, b], axis=2), t, None, poses), 1e-13, label=case)


@pytest.mark.parametrize("case", CASES)
def test_jacobian_transpose_against_the_oracle(case):
    """With root bases J^T w is the efforts of the oracle's inverse dynamics at rest without gravity under the external wrenches -w_k on
    the target bodies (the route of test_twists_and_efforts_against_the_oracle, several bodies at once, one named twice)."""
    sys_, desc = make_case(case)
    m, om = kc.KinModel(desc), OracleModel(desc)
    B = 3
    q, qd = states(sys_, desc, B)
    t = list(range(0, desc.n_joints, 3)) + [desc.n_joints - 1, 0]
    w = cotangents(B, len(t), 6, 63)
    f = np.zeros((B, desc.n_joints, 6))
    for k, body in enumerate(t):
        f[:, body] -= w[:, k]
    z = np.zeros_like(qd)
    close(kv.jacobian_transpose(m, q, w, t), om.rnea(q, z, z, (0.0, 0.0, 0.0), f), 1e-11, label=f"{case} J^T w")


def test_moving_base_takes_the_opposite_wrench():
    """base -> target is root -> target minus root -> base once both wrenches are expressed in the same frame: with the wrench w in the
    target frame, the base receives -w carried into its body-fixed frame."""
    sys_, desc = make_case("humanoid30")
    m = kc.KinModel(desc)
    B, t, b = 2, [19, 12], [6, 23]
    q = states(sys_, desc, B)[0]
    poses = kc.random_poses(np.random.default_rng(64), 2)
    w = cotangents(B, 2, 6, 65)
    got = kv.jacobian_transpose(m, q, w, t, b, poses)
    ref = kv.jacobian_transpose(m, q, w, t, None, poses)
    for r in range(B):
        T0 = kc.joint_frames(m, q[r])
        for k in range(2):
            rel = kc.T_inv(kc.frame_of(m, T0, b[k])) @ kc.frame_of(m, T0, t[k], poses[k])  # the target frame in the base's body-fixed frame
            w_base = kc.Ad(kc.T_inv(rel)).T @ w[r, k]  # a force vector goes target -> base by the transpose of the motion map base -> target
            ref[r] -= kv.jacobian_transpose(m, q[r:r + 1], w_base[None, None], [b[k]])[0]
    close(got, ref, 1e-12, label="moving bases")


@pytest.mark.parametrize("case,scaled", [("arm7", False), ("mixed12", False), ("onedof12", False), ("onedof12", True)])
def test_chart_pullback_against_raw_central_differences(case, scaled):
    """chart_pullback of the checker's gq is the gradient with respect to the RAW q: central differences of sum g . pose along every
    entry of q, with non-unit quaternions (|Q| in 0.8 ... 1.25) in the scaled case -- the poses come from Q / |Q|.  Bound: the 12 K 1e-8
    of the velocity-space differences times the largest factor chart_pullback applies, 2 / |Q| on a quaternion."""
    import torch
    from mecano_amd import autograd
    sys_, desc = make_case(case)
    m = kc.KinModel(desc)
    K, B, eps = 5, 2, 1.0e-5
    t, poses = posed_targets(case, desc, K)
    q = states(sys_, desc, B)[0]
    factor = 2.0
    if scaled:
        quats = [m.cfgs(i)[:4] for i in range(m.n) if int(m.type[i]) in (kc.SIXDOF, kc.SPHERICAL)]
        assert quats
        for ci, s in zip(quats, (0.8, 1.25)):
            q[:, ci] *= s
        factor = 2.0 / 0.8
    g = cotangents(B, K, 12, 66)
    raw = autograd.chart_pullback(desc, torch.tensor(q), torch.tensor(kv.body_poses_vjp(m, q, g, t, poses))).numpy()
    worst = 0.0
    for r in range(B):
        for j in range(desc.nq):
            e = np.zeros(desc.nq)
            e[j] = eps
            d = (loss(m, q[r] + e, g[r], t, poses) - loss(m, q[r] - e, g[r], t, poses)) / (2 * eps)
            worst = max(worst, abs(d - raw[r, j]))
    print(f"{case} scaled={scaled}: worst |difference quotient - chart_pullback| = {worst:.3e}")
    assert worst <= factor * 12 * K * 1.0e-8
    assert np.abs(raw).max() > 0.1
