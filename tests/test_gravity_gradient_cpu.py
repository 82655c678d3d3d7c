"""Pins of the CPU checker of the gravity-gradient calls (tests/gravity_gradient_check.py), and of the names of the two exports on the
host side.  No GPU: the checker is numpy, the references are the C oracle's inverse dynamics and state integrator."""
import os
import re

import numpy as np
import pytest

import gravity_gradient_check as gc
from helpers import build_lump_pair
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem
from oracle.cpu_oracle import OracleModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAVITY = np.array([0.3, -0.2, -9.81])  # not along an axis: every component of the rotated vector is exercised
CASES = ["arm7", "humanoid30", "onedof_tree", "planar", "spherical", "fixed", "lumped"]


def system_of(joints):
    return MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())


def make_case(name, seed=11):
    """(system, desc): the models the device tests use too (tests/test_gpu_gravity_gradient.py imports this)."""
    rng = np.random.default_rng(seed)
    if name == "lumped":  # a revolute + prismatic side subtree, ignored and lumped into the body it hangs from
        root, ignored = build_lump_pair(weld=False)
        sys_ = MultiBodySystem.toMultiBodySystemInput(root, [ignored])
        return sys_, sys_.toModelDesc(considerIgnoredSubtreesInertia=True)
    sys_ = {"arm7": lambda: system_of(rt.nextJointChain(rng, 7)),
            "humanoid30": lambda: rt.nextHumanoid(rng),
            "onedof_tree": lambda: system_of(rt.nextJointTree(rng, 12, ("revolute", "prismatic"))),
            "planar": lambda: system_of(rt.nextJointTree(rng, 7, ("revolute", "planar", "prismatic"))),
            "spherical": lambda: system_of(rt.nextJointTree(rng, 7, ("revolute", "spherical", "prismatic"))),
            "fixed": lambda: system_of(rt.nextJointTree(rng, 9, ("revolute", "fixed", "prismatic")))}[name]()
    return sys_, sys_.toModelDesc()


def random_wrenches(rng, B, n, always=False):
    """[B, n, 6]: about half the configurations carry one to three wrenches of up to 10 N m / 10 N on random bodies, as
    MultiBodyGravityGradientCalculatorTest.java:68-83 does; the others carry none."""
    f = np.zeros((B, n, 6))
    for b in range(B):
        if always or rng.integers(2):
            for _ in range(int(rng.integers(1, 4))):
                f[b, rng.integers(n)] = rng.uniform(-10.0, 10.0, 6)
    return f


def states(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)[0]


def holding_efforts(om, desc, q, f):
    """OracleModel.rnea(q, 0, 0, g, f_ext, False, False), the calculator's tau.  One exception: a body whose centre of mass is off the
    origin of its body-fixed frame -- here only the lumped model's -- takes the oracle down Mecano's offset-CoM Newton-Euler branch, which
    without a twist leaves the moment c x a unscaled by the mass (oracle/mecano_oracle.c: dynamic_wrench, MecanoTools.java:650-692).  The
    gravity calculator has no such branch (it sums m c itself, :463-478), so for that model the Coriolis switch stays on with qd = 0: the
    same efforts, through the branch that scales."""
    z = np.zeros((q.shape[0], desc.nv))
    return om.rnea(q, z, z, GRAVITY, f, bool(np.any(np.asarray(desc.inertia_com) != 0.0)), False)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("with_wrenches", [False, True])
def test_tau_is_inverse_dynamics_with_both_switches_off(case, with_wrenches):
    """MultiBodyGravityGradientCalculatorTest.testGravityMatrixAgainstInverseDynamics: 1e-12, here relative to max(1, |ref|)."""
    sys_, desc = make_case(case)
    om, B = OracleModel(desc), 6
    q = states(sys_, B)
    f = random_wrenches(np.random.default_rng(3), B, desc.n_joints) if with_wrenches else None
    tau, _ = gc.gravity_gradient(desc, q, GRAVITY, f)
    ref = holding_efforts(om, desc, q, f)
    err = np.abs(tau - ref).max()
    print(f"{case}: tau max err {err:.3e}")
    assert err <= 1.0e-12 * max(1.0, np.abs(ref).max())


def fd_column(om, desc, gm, q, f, k, h):
    """Central difference of the inverse dynamics along the integrator's step of unit velocity in DoF k, wrenches held in the world."""
    qd, z = np.zeros((1, gm.nv)), np.zeros((1, gm.nv))
    qd[0, k] = 1.0
    tau = []
    for step in (h, -h):
        q1 = om.integrate(step, q[None], qd, z)[0]
        f1 = None if f is None else gc.wrenches_held_in_world(gm, q, q1[0], f)[None]
        tau.append(holding_efforts(om, desc, q1, f1)[0])
    return (tau[0] - tau[1]) / (2.0 * h)


@pytest.mark.parametrize("case", CASES)
def test_gradient_columns_against_finite_difference(case):
    """Every column against a central difference (h = 1e-5) of OracleModel.rnea along OracleModel.integrate, the wrenches re-expressed
    in the world before the step and matched back to the moved body frames after it.  Bound: the reference test's own 2e-5 absolute
    (compareAgainstFiniteDifference, a forward difference with dq = 1e-7).  Achieved here by the checker: 5.2e-8 at worst (humanoid30,
    entries up to 150; 8.4e-9 on the arm, 9.7e-10 on the 1-DoF tree, 1.3e-9 planar, 4.0e-9 spherical, 1.7e-9 with fixed joints, 4.3e-10
    lumped)."""
    sys_, desc = make_case(case)
    om, gm, B = OracleModel(desc), gc.GravityModel(desc), 2
    q = states(sys_, B)
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    f[1] = 0.0  # the second configuration carries none
    _, grad = gc.gravity_gradient(gm, q, GRAVITY, f)
    worst = 0.0
    for b in range(B):
        for k in range(gm.nv):
            col = fd_column(om, desc, gm, q[b], f[b] if b == 0 else None, k, 1.0e-5)
            worst = max(worst, float(np.abs(col - grad[b][:, k]).max()))
    print(f"{case}: finite-difference max err {worst:.3e}, |grad| up to {np.abs(grad).max():.3g}")
    assert worst <= 2.0e-5


@pytest.mark.parametrize("case", CASES)
def test_unrelated_pairs_are_exactly_zero(case):
    sys_, desc = make_case(case)
    q = states(sys_, 3)
    f = random_wrenches(np.random.default_rng(6), 3, desc.n_joints, always=True)
    _, grad = gc.gravity_gradient(desc, q, GRAVITY, f)
    rel = gc.related(desc)
    assert np.all(grad[:, ~rel] == 0.0)
    if case in ("humanoid30", "onedof_tree"):
        assert (~rel).any()  # the case has branches at all


@pytest.mark.parametrize("case", CASES)
def test_gravity_part_is_symmetric_between_joints(case):
    """Without wrenches the entries of two DoFs of DIFFERENT joints are equal bit for bit (passTwo writes one number to both, :528-533),
    so a model of 1-DoF joints has a symmetric gradient.  Inside one multi-DoF joint the reference evaluates [i][j] and [j][i]
    separately (:500-507) and they differ -- a rotation and a translation of a floating body do not commute; the finite difference above
    confirms the asymmetric block -- so those pairs are left out here."""
    sys_, desc = make_case(case)
    gm = gc.GravityModel(desc)
    _, grad = gc.gravity_gradient(gm, states(sys_, 3), GRAVITY, None)
    same_joint = np.zeros((gm.nv, gm.nv), dtype=bool)
    for k in range(gm.n):
        same_joint[np.ix_(gm.dofs(k), gm.dofs(k))] = True
    asym = grad - grad.transpose(0, 2, 1)
    assert np.all(asym[:, ~same_joint] == 0.0)
    if all(len(gm.dofs(k)) <= 1 for k in range(gm.n)):
        assert np.all(asym == 0.0)


def test_wrenches_touch_descendant_rows_only_and_flip_sign_inside_a_joint():
    """The external part goes to [descendant][ancestor] only, and with opposite signs to the two entries of a pair of DoFs of one joint."""
    sys_, desc = make_case("humanoid30")
    gm = gc.GravityModel(desc)
    q = states(sys_, 2)
    f = random_wrenches(np.random.default_rng(8), 2, gm.n, always=True)
    _, g0 = gc.gravity_gradient(gm, q, GRAVITY, None)
    _, g1 = gc.gravity_gradient(gm, q, GRAVITY, f)
    ext = g1 - g0
    assert np.abs(ext).max() > 1.0
    for k in range(gm.n):
        a = gm.parent[k]
        while a >= 0:
            assert np.all(ext[:, gm.dofs(a)[:, None], gm.dofs(k)[None, :]] == 0.0)  # [ancestor][descendant]
            a = gm.parent[a]
        blk = ext[:, gm.dofs(k)[:, None], gm.dofs(k)[None, :]]
        assert np.abs(blk + blk.transpose(0, 2, 1)).max() <= 1e-12 * max(1.0, np.abs(blk).max())


def test_lumped_subtree_equals_welded_subtree():
    """Ignored joints lumped into their parent (updateIgnoredSubtreeInertia, :262-290) give what the same bodies welded on give."""
    _, lumped = make_case("lumped")
    root, _ = build_lump_pair(weld=True)
    welded = MultiBodySystem.toMultiBodySystemInput(root).toModelDesc()
    assert lumped.nv == welded.nv == 3 and lumped.nq == welded.nq
    q = np.random.default_rng(2).uniform(-1.0, 1.0, (4, lumped.nq))
    t0, g0 = gc.gravity_gradient(lumped, q, GRAVITY, None)
    t1, g1 = gc.gravity_gradient(welded, q, GRAVITY, None)
    assert np.abs(t0 - t1).max() <= 1e-12 * max(1.0, np.abs(t1).max())
    assert np.abs(g0 - g1).max() <= 1e-12 * max(1.0, np.abs(g1).max())


def test_checker_joint_poses_are_featherstone_np_s():
    """The checker's frames against oracle/featherstone_np.py's own child-to-parent transforms, for the joint kinds that module has."""
    from oracle import featherstone_np as fnp
    sys_ = system_of(rt.nextJointTree(np.random.default_rng(9), 10, ("revolute", "prismatic", "sixdof", "fixed")))
    desc = sys_.toModelDesc()
    fm, gm = fnp.Model(desc), gc.GravityModel(desc)
    q = states(sys_, 1)[0]
    for i in range(gm.n):
        Rb, pb = gm.Xb[i, :9].reshape(3, 3), gm.Xb[i, 9:]
        RJ, pJ = gm.joint_pose(i, q)
        assert np.abs(fnp.plucker_motion(Rb, pb) @ fnp.plucker_motion(RJ, pJ) - fm.X_child_to_parent(i, q)).max() <= 1e-15


def test_exports_are_named_on_every_host_side():
    """include/mecano_hip.h, the ctypes symbol list and the Panama binding all carry the two exports."""
    from mecano_amd import _lib
    header = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
    native = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
    for name in ("mh_gravity_gradient_f64", "mh_gravity_gradient_f32"):
        assert re.search(r"\bmh_status\s+%s\s*\(" % name, header), name
        assert name in _lib.ABI_SYMBOLS, name
        assert re.search(r'handle\(\s*"%s"' % name, native), name
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", header)  # purely additive
