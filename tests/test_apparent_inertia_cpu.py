"""Pins of the CPU checker of the apparent-inertia calls (tests/apparent_inertia_check.py) by facts that do not come from the call it is
built on, and the case builders the device tests share.  No GPU: the checker is numpy on top of the C oracle."""
import zlib

import numpy as np
import pytest

import apparent_inertia_check as ac
from helpers import build_lump_pair, close
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem
from oracle.cpu_oracle import OracleModel

# the families of tests/test_response.py, then the arm, the humanoid, the 128-body tree, a lumped model and one with two locked joints
RANDOM_FAMILIES = {
    "prismatic_chain": lambda rng, n: rt.nextJointChain(rng, n, ("prismatic",)),
    "revolute_tree": lambda rng, n: rt.nextJointTree(rng, n, ("revolute",)),
    "onedof_tree": lambda rng, n: rt.nextJointTree(rng, n, ("revolute", "prismatic")),
    "floating_revolute_chain": lambda rng, n: rt.nextFloatingChain(rng, n, ("revolute",)),
    "mixed_tree": lambda rng, n: rt.nextJointTree(rng, n, ("revolute", "prismatic", "sixdof", "fixed", "planar", "spherical")),
}
CASES = sorted(RANDOM_FAMILIES) + ["arm7", "humanoid30", "tree128", "lumped", "locked2"]
WELL_CONDITIONED = ("arm7", "humanoid30")  # cond_inf(H) <= 420 on the humanoid: the standing 1e-10 holds; everything else scales with cond(H)
HUMANOID_TARGETS = [6, 12, 19, 23]  # both feet, both hands


def system_of(joints):
    return MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())


def make_case(name):
    """(system, desc, locked flags per joint or None)"""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 3)
    locked = None
    if name in RANDOM_FAMILIES:
        sys_ = system_of(RANDOM_FAMILIES[name](rng, 14))
    elif name == "arm7":
        sys_ = rt.committedBenchmarkSystems()["arm7"]
    elif name in ("humanoid30", "locked2"):
        sys_ = rt.nextHumanoid(np.random.default_rng(43))
    elif name == "tree128":
        sys_ = rt.committedBenchmarkSystems()["tree128"]
    elif name == "lumped":
        root, ignored = build_lump_pair(weld=False)
        sys_ = MultiBodySystem.toMultiBodySystemInput(root, [ignored])
        return sys_, sys_.toModelDesc(considerIgnoredSubtreesInertia=True), None
    desc = sys_.toModelDesc()
    if name == "locked2":  # a knee and a shoulder joint as acceleration sources
        locked = np.zeros(desc.n_joints, dtype=np.int32)
        locked[[4, 16]] = 1
    return sys_, desc, locked


def states(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)[0]


def targets_of(name, desc, K, seed=1):
    """K target joints: the humanoid's feet and hands first, otherwise random ones; with K >= 3 the second target is named twice."""
    rng = np.random.default_rng(seed + K)
    if name in ("humanoid30", "locked2") and K == 4:
        return list(HUMANOID_TARGETS)
    t = [int(v) for v in rng.integers(0, desc.n_joints, K)]
    if K >= 3:
        t[-1] = t[1]
    return t


def test_motion_and_force_transforms_are_dual():
    rng = np.random.default_rng(0)
    pose = ac.random_poses(rng, 1)[0]
    M = ac.motion_into_frame(pose)
    R, p = pose[:9].reshape(3, 3), pose[9:]
    n, f = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    w_body = M.T @ np.concatenate([n, f])
    assert np.allclose(w_body[3:], R @ f, atol=1e-15) and np.allclose(w_body[:3], R @ n + np.cross(p, R @ f), atol=1e-15)


@pytest.mark.parametrize("case", [c for c in CASES if c != "locked2"])
def test_two_routes_agree(case):
    """(i) forward dynamics' own body accelerations against forward dynamics followed by the Newton-Euler sweep's."""
    sys_, desc, _ = make_case(case)
    om, B = OracleModel(desc), 2 if case == "tree128" else 4
    q = states(sys_, B)
    t = targets_of(case, desc, 4)
    W1 = ac.apparent_inertia_inverse(om, q, t, coupled=True)
    W2 = ac.apparent_inertia_inverse(om, q, t, coupled=True, second_route=True)
    bounds = ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED) * 10.0  # two oracle calls are compared
    ac.close_rows(W2, W1, bounds, label=case)
    if case == "humanoid30":
        assert np.abs(W1 - W2).max() < 1.0e-9


@pytest.mark.parametrize("case", CASES)
def test_symmetric_and_positive(case):
    """(ii) W = J H^-1 J^T: symmetric, positive semi-definite; definite when the targets are distinct bodies that can all move freely --
    asserted on the humanoid's feet and hands."""
    sys_, desc, locked = make_case(case)
    om, B = OracleModel(desc), 2 if case == "tree128" else 8
    q = states(sys_, B)
    t = targets_of(case, desc, 4)
    W = ac.apparent_inertia_inverse(om, q, t, ac.random_poses(np.random.default_rng(2), 4), coupled=True, locked=locked)
    scale = max(1.0, np.abs(W).max())
    conds = ac.mass_matrix_conds(om, q).max()
    asym = np.abs(W - W.transpose(0, 2, 1)).max()
    print(f"{case}: asymmetry {asym:.3e}, largest entry {np.abs(W).max():.3e}, cond(H) <= {conds:.3e}")
    assert asym <= 1.0e-10 * scale * max(1.0, conds / 420.0)
    eig = np.linalg.eigvalsh(0.5 * (W + W.transpose(0, 2, 1)))
    assert eig.min() >= -1.0e-10 * scale * max(1.0, conds / 420.0)
    if case == "humanoid30":
        assert eig.min() > 1.0e-6 and asym < 1.0e-13  # definite: nine orders above the rounding of entries of size 1


@pytest.mark.parametrize("case", [c for c in CASES if c != "locked2"])
def test_linearity_in_the_full_forward_dynamics(case):
    """(iii) MultiBodyResponseCalculatorTest.java:301-344: forward dynamics with the test wrenches minus forward dynamics without them, at
    random velocities, efforts, gravity and standing wrenches, is W applied to the test wrenches."""
    sys_, desc, _ = make_case(case)
    om, B, K = OracleModel(desc), 2 if case == "tree128" else 5, 3
    rng = np.random.default_rng(4)
    q, qd, _, tau = rt.nextState(rng, sys_, B)
    t = targets_of(case, desc, K)
    poses = ac.random_poses(rng, K)
    W = ac.apparent_inertia_inverse(om, q, t, poses, coupled=True)
    g = (0.4, -0.1, -7.3)
    f = rng.uniform(-5, 5, (B, desc.n_joints, 6))
    w = rng.uniform(-5, 5, (B, K, 6))  # in the targets' frames
    fw = f.copy()
    for k, j in enumerate(t):
        fw[:, j] += w[:, k] @ ac.motion_into_frame(poses[k])  # row vector times M = M^T times the column
    _, acc1, _ = om.aba_bodies(q, qd, tau, g, fw)
    _, acc0, _ = om.aba_bodies(q, qd, tau, g, f)
    got = np.stack([(acc1 - acc0)[:, j] @ ac.motion_into_frame(poses[k]).T for k, j in enumerate(t)], axis=1).reshape(B, 6 * K)
    ref = np.einsum("bij,bj->bi", W, w.reshape(B, 6 * K))
    bounds = ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED) * 100.0  # a difference of two accelerations of size |g| + |f|
    ac.close_rows(got, ref, bounds, label=case)


def test_point_response_to_a_pure_force_by_hand():
    """(iv) a frame displaced by p without rotation: a force f at the point is the wrench (p x f, f) on the body, and the point accelerates
    with a + alpha x p."""
    sys_, desc, _ = make_case("humanoid30")
    om, B = OracleModel(desc), 4
    q = states(sys_, B)
    p = np.array([0.11, -0.07, 0.23])
    pose = np.concatenate([np.eye(3).reshape(9), p])
    j = HUMANOID_TARGETS[2]
    W = ac.apparent_inertia_inverse(om, q, [j], pose[None])[:, 0]
    Wb = ac.body_frame_columns(om, q, j)[:, j]
    by_hand = np.zeros((B, 3, 3))
    for c in range(3):
        f = np.zeros(3)
        f[c] = 1.0
        a = Wb @ np.concatenate([np.cross(p, f), f])
        by_hand[:, :, c] = a[:, 3:] + np.cross(a[:, :3], p)
    close(W[:, 3:, 3:], by_hand, 1.0e-12)


def test_single_free_body_in_closed_form():
    """(v) one SixDoF joint: W is the inverse of the body's spatial inertia about the body-fixed frame, whatever q."""
    rng = np.random.default_rng(8)
    from mecano_amd.multibody import RigidBody
    root = RigidBody("root")
    joint = rt.nextSixDoFJoint(rng, "free", root)
    rt.nextRigidBody(rng, "body", joint)
    sys_ = MultiBodySystem.toMultiBodySystemInput(root)
    desc = sys_.toModelDesc()
    om, B = OracleModel(desc), 3
    q = states(sys_, B)
    m, c, J = float(desc.inertia_mass[0]), np.asarray(desc.inertia_com).reshape(-1, 3)[0], np.asarray(desc.inertia_J).reshape(-1, 3, 3)[0]
    I6 = np.zeros((6, 6))
    I6[:3, :3], I6[:3, 3:], I6[3:, :3], I6[3:, 3:] = J, m * ac.skew(c), -m * ac.skew(c), m * np.eye(3)
    W = ac.apparent_inertia_inverse(om, q, [0])[:, 0]
    close(W, np.broadcast_to(np.linalg.inv(I6), W.shape), 1.0e-10)


def test_humanoid_numbers_of_the_bound():
    """What the 1e-10 bound on the humanoid rests on: largest entry about 1, smallest eigenvalue 2e-3, cond(H) <= 420."""
    sys_, desc, _ = make_case("humanoid30")
    om = OracleModel(desc)
    q = states(sys_, 8)
    W = ac.apparent_inertia_inverse(om, q, HUMANOID_TARGETS, coupled=True)
    assert np.abs(W).max() < 10.0 and ac.mass_matrix_conds(om, q).max() < 2000.0


def test_locked_joints_keep_a_zero_change():
    """An acceleration-source joint between the root and the target changes the response; locking every joint of the path to a fixed-base
    target leaves no response at all."""
    sys_, desc, locked = make_case("locked2")
    om, B = OracleModel(desc), 3
    q = states(sys_, B)
    W_free = ac.apparent_inertia_inverse(om, q, HUMANOID_TARGETS, coupled=True)
    W_locked = ac.apparent_inertia_inverse(om, q, HUMANOID_TARGETS, coupled=True, locked=locked)
    assert np.abs(W_free - W_locked).max() > 1.0e-3
    assert np.abs(W_locked - W_locked.transpose(0, 2, 1)).max() < 1.0e-12
    arm_sys, arm, _ = make_case("arm7")
    W0 = ac.apparent_inertia_inverse(OracleModel(arm), states(arm_sys, 2), [6], locked=np.ones(7, dtype=np.int32))
    assert np.abs(W0).max() == 0.0
