"""Pins of the CPU checker of mh_mass_matrix_inverse_* (tests/mass_matrix_inverse_check.py) by facts that do not come from the call it
is built on.  No GPU: the checker is numpy on top of the C oracle.  The cases are those of tests/test_apparent_inertia_cpu.py."""
import numpy as np
import pytest

import apparent_inertia_check as ac
import mass_matrix_inverse_check as mc
from helpers import close
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem, RigidBody
from oracle.cpu_oracle import OracleModel
from test_apparent_inertia_cpu import CASES, WELL_CONDITIONED, make_case, states, system_of


def batch_of(case):
    return 2 if case == "tree128" else 8


@pytest.mark.parametrize("case", CASES)
def test_is_the_inverse_of_the_mass_matrix(case):
    """Against a dense inverse of the oracle's CRBA, and H H^-1 = I, per configuration within apparent_inertia_check.bound_of.  With
    acceleration-source joints: rows and columns of their DoFs are exactly zero, the rest is the inverse of H restricted to the others."""
    sys_, desc, locked = make_case(case)
    om, B = OracleModel(desc), batch_of(case)
    q = states(sys_, B)
    Hinv = mc.mass_matrix_inverse(om, q, None, locked)
    H = om.crba(q)
    held, free = mc.locked_dofs(desc, locked)
    ref = np.zeros_like(H)
    ref[np.ix_(range(B), free, free)] = np.linalg.inv(H[np.ix_(range(B), free, free)])
    bounds = ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED)
    ac.close_rows(Hinv, ref, bounds, label=f"{case} against inv(crba)")
    eye = np.zeros_like(H)
    eye[:, free, free] = 1.0
    prod = np.zeros_like(H)
    prod[np.ix_(range(B), free, free)] = H[np.ix_(range(B), free, free)] @ Hinv[np.ix_(range(B), free, free)]
    ac.close_rows(prod, eye, bounds, label=f"{case} H Hinv = 1")
    if held:
        assert not Hinv[:, held, :].any() and not Hinv[:, :, held].any()
        assert np.abs(Hinv[np.ix_(range(B), free, free)] - ref[np.ix_(range(B), free, free)]).max() < 1.0e-13 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("case", CASES)
def test_symmetric(case):
    """Every column is a forward-dynamics call of its own, so symmetry is a fact about the checker, relative to the largest entry of the
    configuration (tree128's entries reach 3.8e3)."""
    sys_, desc, locked = make_case(case)
    om, B = OracleModel(desc), batch_of(case)
    q = states(sys_, B)
    Hinv = mc.mass_matrix_inverse(om, q, None, locked)
    ac.close_rows(Hinv, Hinv.transpose(0, 2, 1), ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED), label=f"{case} symmetry")
    if case == "humanoid30":
        assert np.abs(Hinv - Hinv.transpose(0, 2, 1)).max() < 1.0e-13


@pytest.mark.parametrize("case", ["mixed_tree", "humanoid30", "locked2"])
def test_listed_columns_are_columns_of_the_full_matrix(case):
    sys_, desc, locked = make_case(case)
    om = OracleModel(desc)
    q = states(sys_, 3)
    cols = mc.column_list(desc)
    assert len(set(cols)) < len(cols) <= 64
    full = mc.mass_matrix_inverse(om, q, None, locked)
    assert np.array_equal(mc.mass_matrix_inverse(om, q, cols, locked), full[:, :, cols])


def test_single_free_body_in_closed_form():
    """One SixDoF joint: H is the body's 6 x 6 spatial inertia in the frame after the joint, whatever q: the inertia of the body-fixed
    frame (desc.inertia_*) carried there by the constant pose desc.X_com."""
    rng = np.random.default_rng(8)
    root = RigidBody("root")
    joint = rt.nextSixDoFJoint(rng, "free", root)
    rt.nextRigidBody(rng, "body", joint)
    sys_ = MultiBodySystem.toMultiBodySystemInput(root)
    desc = sys_.toModelDesc()
    om = OracleModel(desc)
    q = states(sys_, 3)
    m, c, J = float(desc.inertia_mass[0]), np.asarray(desc.inertia_com).reshape(-1, 3)[0], np.asarray(desc.inertia_J).reshape(-1, 3, 3)[0]
    I6 = np.zeros((6, 6))
    I6[:3, :3], I6[:3, 3:], I6[3:, :3], I6[3:, 3:] = J, m * ac.skew(c), -m * ac.skew(c), m * np.eye(3)
    M = ac.motion_into_frame(np.asarray(desc.X_com, dtype=np.float64).reshape(-1, 12)[0])  # twist of the joint frame -> body-fixed frame
    Hinv = mc.mass_matrix_inverse(om, q)
    close(Hinv, np.broadcast_to(np.linalg.inv(M.T @ I6 @ M), Hinv.shape), 1.0e-10)


def test_prismatic_chain_last_column_by_hand():
    """Prismatic joints only: nothing rotates, so H[i][j] = (a_i . a_j) M_max(i, j) with a_i the axis of joint i in the world and M_k the
    mass outboard of joint k -- whatever q and wherever the centres of mass are.  Solved here by hand-built H; the last column is also the
    forward dynamics of a unit force at the tip."""
    rng = np.random.default_rng(12)
    n = 5
    sys_ = system_of(rt.nextJointChain(rng, n, ("prismatic",)))
    desc = sys_.toModelDesc()
    om = OracleModel(desc)
    q = states(sys_, 4)
    # world axes from the oracle itself would be the call under test; the Newton-Euler sweep gives them instead: the linear acceleration
    # of the last body per unit acceleration of joint i is a_i in that body's frame (no rotation between prismatic joints' bodies but the
    # constant ones, which the sweep carries)
    z = np.zeros((q.shape[0], n))
    axes = np.zeros((q.shape[0], n, 3))
    for i in range(n):
        e = z.copy()
        e[:, i] = 1.0
        axes[:, i] = om.rnea_bodies(q, z, e, (0.0, 0.0, 0.0))[1][:, n - 1, 3:]
    masses = np.asarray(desc.inertia_mass, dtype=np.float64)
    outboard = np.array([masses[k:].sum() for k in range(n)])
    H = np.einsum("bik,bjk->bij", axes, axes) * outboard[np.maximum.outer(np.arange(n), np.arange(n))]
    close(om.crba(q), H, 1.0e-12)
    Hinv = mc.mass_matrix_inverse(om, q)
    close(Hinv[:, :, n - 1], np.linalg.solve(H, np.broadcast_to(np.eye(n)[:, n - 1:], (q.shape[0], n, 1)))[:, :, 0], 1.0e-10)
    close(Hinv, np.linalg.inv(H), 1.0e-10)


def test_every_joint_locked_gives_zeros():
    arm_sys, arm, _ = make_case("arm7")
    Hinv = mc.mass_matrix_inverse(OracleModel(arm), states(arm_sys, 2), None, np.ones(7, dtype=np.int32))
    assert Hinv.shape == (2, 7, 7) and not Hinv.any()
