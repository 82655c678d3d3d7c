"""Pins of the CPU checker of the kinematics calls (tests/kinematics_check.py) by facts that do not come from its own composition of
transforms -- differences of poses, the dense body Jacobians of oracle/featherstone_np.py, the C oracle's dynamics, one closed form -- and
the case builders the device tests share.  No GPU."""
import zlib

import numpy as np
import pytest

import apparent_inertia_check as ac
import kinematics_check as kc
from helpers import close
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem, RevoluteJoint, RigidBody
from oracle import featherstone_np as fnp
from oracle.cpu_oracle import OracleModel

HUMANOID_TARGETS = [6, 12, 19, 23]  # both feet, both hands
CASES = ["arm7", "humanoid30", "mixed12", "onedof12"]
DENSE_CASES = ["arm7", "humanoid30", "onedof12"]  # the joint kinds oracle/featherstone_np.py has


def make_case(name):
    """(system, desc).  mixed12: a random tree of revolute, prismatic, planar, spherical and fixed joints with one subtree ignored and
    shuffled index maps; onedof12: revolute, prismatic, floating and fixed joints with shuffled index maps."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 11)
    if name == "arm7":
        sys_ = rt.committedBenchmarkSystems()["arm7"]
        return sys_, sys_.toModelDesc()
    if name == "humanoid30":
        sys_ = rt.nextHumanoid(np.random.default_rng(43))
        return sys_, sys_.toModelDesc()
    if name == "tree128":
        sys_ = rt.committedBenchmarkSystems()["tree128"]
        return sys_, sys_.toModelDesc()
    if name == "mixed12":
        for salt in range(100):  # the first draw in which every kind is among the twelve joints that stay
            rng = np.random.default_rng(zlib.crc32(name.encode()) + 11 + salt)
            joints = rt.nextJointTree(rng, 13, ("revolute", "prismatic", "planar", "spherical", "fixed", "revolute"))
            sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor(), [joints[-1]])
            kept = sys_.getJointsToConsider()
            if len(kept) == 12 and {j.joint_type for j in kept} == {0, 1, 3, 4, 5}:
                break
        else:
            raise AssertionError("no draw with every joint kind")
    elif name == "onedof12":
        joints = rt.nextJointTree(rng, 12, ("revolute", "prismatic", "sixdof", "fixed", "revolute"))
        sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
    else:
        raise KeyError(name)
    desc = sys_.toModelDesc()
    perm_v, perm_q = rng.permutation(desc.nv).astype(np.int32), rng.permutation(desc.nq).astype(np.int32)
    desc.dof_indices = perm_v[np.asarray(desc.dof_indices)]
    desc.cfg_indices = perm_q[np.asarray(desc.cfg_indices)]
    return sys_, desc


def states(sys_, desc, B, seed=5):
    """(q, qd) in the index space of desc (the system's own provider numbers the rows in joint order; desc may have shuffled them)."""
    q0, qd0, _, _ = rt.nextState(np.random.default_rng(seed), sys_, B)
    plain = sys_.toModelDesc()
    q, qd = np.zeros((B, desc.nq)), np.zeros((B, desc.nv))
    q[:, np.asarray(desc.cfg_indices)] = q0[:, np.asarray(plain.cfg_indices)]
    qd[:, np.asarray(desc.dof_indices)] = qd0[:, np.asarray(plain.dof_indices)]
    return q, qd


def targets_of(name, desc, K, seed=1):
    """(targets, bases): the humanoid's feet and hands first, with bases = the root, the left foot, the root, the right hand (a
    foot-to-hand and a hand-to-hand chain cross the common ancestor); otherwise random ones, -1 among them; with K >= 3 the second
    target is named twice."""
    rng = np.random.default_rng(seed + K)
    if name == "humanoid30" and K == 4:
        return list(HUMANOID_TARGETS), [-1, 6, -1, 19]
    t = [int(v) for v in rng.integers(0, desc.n_joints, K)]
    b = [int(v) for v in rng.integers(-1, desc.n_joints, K)]
    if K >= 3:
        t[-1] = t[1]
    if K >= 2:
        b[0] = -1
    return t, b


def test_cases_are_what_they_claim():
    _, d = make_case("mixed12")
    kinds = set(int(t) for t in d.joint_type)
    assert {kc.PRISMATIC, kc.PLANAR, kc.SPHERICAL, kc.FIXED} <= kinds and d.n_joints == 12
    assert not np.array_equal(d.dof_indices, np.arange(d.nv))
    _, d = make_case("onedof12")
    assert set(int(t) for t in d.joint_type) <= {kc.REVOLUTE, kc.PRISMATIC, kc.SIXDOF, kc.FIXED} and d.n_joints == 12


def test_checker_transforms_are_featherstone_np_s():
    """KinModel defers to featherstone_np.Model for the joint kinds that module has, and the 4 x 4 <-> 6 x 6 conversions are inverse."""
    sys_, desc = make_case("onedof12")
    fm, km = fnp.Model(desc), kc.KinModel(desc)
    q = states(sys_, desc, 1)[0][0]
    for i in range(desc.n_joints):
        X = fm.X_child_to_parent(i, q)
        assert np.array_equal(km.X_child_to_parent(i, q), X) and np.array_equal(km.S(i), fm.S(i))
        assert np.abs(kc.Ad(kc.T_of_plucker(X)) - X).max() <= 1e-15


@pytest.mark.parametrize("case", CASES)
def test_pose_differences_reproduce_the_jacobian(case):
    """(pose(q (+) eps e_j) - pose(q (-) eps e_j)) / 2 eps, as a twist of the target frame relative to the base, is column j of J: for
    every DoF index, root and non-root bases, non-identity poses.  eps = 1e-5: truncation eps^2, rounding 1e-16 / eps."""
    sys_, desc = make_case(case)
    m = kc.KinModel(desc)
    K = 4
    t, b = targets_of(case, desc, K)
    poses = kc.random_poses(np.random.default_rng(3), K)
    q = states(sys_, desc, 2)[0]
    J, _ = kc.geometric_jacobian(m, q, t, b, poses)
    eps = 1.0e-5

    def relative(qv, k):
        T0 = kc.joint_frames(m, qv)
        return kc.T_inv(kc.frame_of(m, T0, b[k])) @ kc.frame_of(m, T0, t[k], poses[k])

    worst = 0.0
    for r in range(q.shape[0]):
        for j in range(desc.nv):
            e = np.zeros(desc.nv)
            e[j] = eps
            qp, qm = kc.configuration_add(m, q[r], e), kc.configuration_add(m, q[r], -e)
            for k in range(K):
                tw = kc.twist_of_difference(relative(qm, k), relative(qp, k), relative(q[r], k), eps)
                worst = max(worst, np.abs(tw - J[r, 6 * k:6 * k + 6, j]).max())
    print(f"{case}: worst |difference quotient - J| = {worst:.3e}")
    assert worst <= 1.0e-8
    assert np.abs(J).max() > 0.1


@pytest.mark.parametrize("case", DENSE_CASES)
def test_jacobian_against_dense_body_jacobians(case):
    """Root bases, identity poses: J_k brought from the body-fixed frame to the frame after the joint is featherstone_np's J of that body."""
    sys_, desc = make_case(case)
    m, fm = kc.KinModel(desc), fnp.Model(desc)
    q, qd = states(sys_, desc, 2)
    t = list(range(desc.n_joints))
    for r in range(2):
        J, _ = kc.geometric_jacobian(m, q[r:r + 1], t)
        _, J_dense, _, _ = fnp._body_jacobians(fm, q[r], qd[r])
        for k in t:
            to_joint_frame = kc.Ad(kc.T_of12(m.Xc[k]))
            close(to_joint_frame @ J[0, 6 * k:6 * k + 6], J_dense[k], 1e-12, label=case)


@pytest.mark.parametrize("case", CASES)
def test_twists_and_efforts_against_the_oracle(case):
    """J qd is the body twist of the oracle's Newton-Euler sweep (re-expressed in the pose), and J^T w the efforts of its inverse dynamics
    at rest without gravity under the external wrench -w."""
    sys_, desc = make_case(case)
    m, om = kc.KinModel(desc), OracleModel(desc)
    B = 3
    q, qd = states(sys_, desc, B)
    t = list(range(desc.n_joints))
    poses = kc.random_poses(np.random.default_rng(4), len(t))
    _, _, twists = om.rnea_bodies(q, qd, np.zeros_like(qd), (0.0, 0.0, 0.0))
    J0, _ = kc.geometric_jacobian(m, q, t)
    Jp, _ = kc.geometric_jacobian(m, q, t, None, poses)
    rng = np.random.default_rng(6)
    for k in t:
        close(np.einsum("bij,bj->bi", J0[:, 6 * k:6 * k + 6], qd), twists[:, k], 1e-11, label=f"{case} J qd")
        M = kc.motion_into_frame(poses[k])
        close(np.einsum("bij,bj->bi", Jp[:, 6 * k:6 * k + 6], qd), twists[:, k] @ M.T, 1e-11, label=f"{case} J qd, posed")
    for k in t[::3]:
        w = rng.uniform(-1, 1, 6)
        f = np.zeros((B, desc.n_joints, 6))
        f[:, k] = -w
        z = np.zeros_like(qd)
        tau = om.rnea(q, z, z, (0.0, 0.0, 0.0), f)
        close(np.einsum("bji,j->bi", J0[:, 6 * k:6 * k + 6], w), tau, 1e-11, label=f"{case} J^T w")


@pytest.mark.parametrize("case", CASES)
def test_convective_term_against_relative_acceleration(case):
    """The convective term against the oracle's RigidBodyAccelerationProvider.getRelativeAcceleration at qdd = 0 (gravity cancels in a
    relative acceleration), for root and non-root bases -- on the humanoid foot to hand, across the common ancestor -- and re-expressed
    in the target pose."""
    sys_, desc = make_case(case)
    m, om = kc.KinModel(desc), OracleModel(desc)
    B, K = 3, 4
    q, qd = states(sys_, desc, B)
    t, b = targets_of(case, desc, K)
    if case == "humanoid30":
        assert (b[1], t[1]) == (6, 12) and kc.joint_chain(m, 6, 19)[0][1] == -1.0
        t, b = t + [19], b + [6]  # left foot -> left hand
    poses = kc.random_poses(np.random.default_rng(7), len(t))
    rel = om.relative_acceleration(q, qd, np.zeros_like(qd), b, t)
    _, c0 = kc.geometric_jacobian(m, q, t, b, None, qd)
    _, cp = kc.geometric_jacobian(m, q, t, b, poses, qd)
    assert np.abs(c0).max() > 0.1
    for k in range(len(t)):
        if t[k] < 0:
            continue
        close(c0[:, k], rel[:, k], 1e-11, label=f"{case} convective")
        close(cp[:, k], rel[:, k] @ kc.motion_into_frame(poses[k]).T, 1e-11, label=f"{case} convective, posed")


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_J_Hinv_JT_is_the_apparent_inertia_inverse(case):
    sys_, desc = make_case(case)
    m, om = kc.KinModel(desc), OracleModel(desc)
    B, K = 3, 4
    q = states(sys_, desc, B)[0]
    t, _ = targets_of(case, desc, K)
    poses = kc.random_poses(np.random.default_rng(8), K)
    J, _ = kc.geometric_jacobian(m, q, t, None, poses)
    H = om.crba(q)
    W = np.stack([J[r] @ np.linalg.inv(H[r]) @ J[r].T for r in range(B)])
    ac.close_rows(W, ac.apparent_inertia_inverse(om, q, t, poses, coupled=True), ac.bound_of(om, q, desc.n_joints, True), label=case)


def test_planar_two_link_arm_closed_form():
    l1, l2 = 0.7, 0.45
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    root = RigidBody("base")
    j1 = RevoluteJoint("j1", root, None, (0.0, 0.0, 1.0))
    b1 = RigidBody("b1", j1, np.eye(3), 1.0, inertiaPose=ident)
    j2 = RevoluteJoint("j2", b1, (np.eye(3), np.array([l1, 0.0, 0.0])), (0.0, 0.0, 1.0))
    RigidBody("b2", j2, np.eye(3), 1.0, inertiaPose=ident)
    desc = MultiBodySystem.toMultiBodySystemInput(root).toModelDesc()
    m = kc.KinModel(desc)
    q = np.array([[0.3, -1.1], [2.0, 0.4]])
    qd = np.array([[0.8, -0.5], [-1.2, 0.9]])
    tip = np.concatenate([np.eye(3).reshape(9), [l2, 0.0, 0.0]])
    P = kc.body_poses(m, q, [1], tip[None])
    J, c = kc.geometric_jacobian(m, q, [1], None, tip[None], qd)
    for r in range(2):
        q1, q2 = q[r]
        c1, s1, c12, s12 = np.cos(q1), np.sin(q1), np.cos(q1 + q2), np.sin(q1 + q2)
        R = np.array([[c12, -s12, 0.0], [s12, c12, 0.0], [0.0, 0.0, 1.0]])
        assert np.abs(P[r, 0, :9].reshape(3, 3) - R).max() <= 1e-15
        assert np.abs(P[r, 0, 9:] - np.array([l1 * c1 + l2 * c12, l1 * s1 + l2 * s12, 0.0])).max() <= 1e-15
        v1 = R.T @ np.array([-l1 * s1 - l2 * s12, l1 * c1 + l2 * c12, 0.0])
        v2 = R.T @ np.array([-l2 * s12, l2 * c12, 0.0])
        ref = np.array([[0, 0], [0, 0], [1, 1], [v1[0], v2[0]], [v1[1], v2[1]], [0, 0]])
        assert np.abs(J[r] - ref).max() <= 1e-15
        lin = qd[r, 0] * qd[r, 1] * np.array([l1 * np.cos(q2), -l1 * np.sin(q2), 0.0])
        assert np.abs(c[r, 0] - np.concatenate([np.zeros(3), lin])).max() <= 1e-15
