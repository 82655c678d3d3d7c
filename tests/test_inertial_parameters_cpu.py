"""Pins of the CPU checker of the per-configuration inertial-parameter calls (tests/inertial_parameters_check.py).  None of them comes
from the call under test: the references are the C oracle on the unmodified description, its regressor, and its own round trip."""
import numpy as np
import pytest

import inertial_parameters_check as ipc
from helpers import build_lump_pair, close_aba
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem
from oracle.cpu_oracle import OracleModel

GRAVITY = np.array([0.3, -0.2, -9.81])
CASES = ["arm7", "humanoid30", "mixed", "lumped"]


def make_case(name, seed=17):
    """(system, desc) of the four models the device tests use too (tests/test_gpu_inertial_parameters.py imports this)."""
    rng = np.random.default_rng(seed)
    if name == "lumped":  # a revolute + prismatic side subtree, ignored and lumped into the body it hangs from
        root, ignored = build_lump_pair(weld=False)
        sys_ = MultiBodySystem.toMultiBodySystemInput(root, [ignored])
        return sys_, sys_.toModelDesc(considerIgnoredSubtreesInertia=True)
    if name == "arm7":
        sys_ = MultiBodySystem.toMultiBodySystemInput(rt.nextJointChain(rng, 7)[0].getPredecessor())
    elif name == "humanoid30":
        sys_ = rt.nextHumanoid(rng)
    else:  # one random mixed tree: planar, spherical and fixed joints (whose successors carry inertia) among 1-DoF ones
        joints = rt.nextJointTree(np.random.default_rng(21), 11, ("revolute", "planar", "fixed", "spherical", "prismatic"))  # a seed with all five
        sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
    desc = sys_.toModelDesc()
    assert name != "mixed" or {0, 1, 3, 4, 5} <= {int(t) for t in desc.joint_type}
    return sys_, desc


def batch(sys_, desc, B, seed=3):
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(seed), sys_, B)
    pi = ipc.physical_parameter_sets(desc, np.random.default_rng(seed + 1), B)
    return q, qd, qdd, tau, pi


@pytest.mark.parametrize("case", CASES)
def test_generated_parameter_sets_are_physical(case):
    _, desc = make_case(case)
    for pi in ipc.physical_parameter_sets(desc, np.random.default_rng(2), 3):
        for row, own in zip(pi, ipc.parameters_of(desc)):
            m, c = row[0], row[1:4]
            J = np.array([[row[4], row[5], row[6]], [row[5], row[7], row[8]], [row[6], row[8], row[9]]])
            Jc = J - m * (c @ c * np.eye(3) - np.outer(c, c))
            ev = np.linalg.eigvalsh(Jc)
            if own[0] > 0.0:
                assert m > 0.0 and ev[0] > 0.0  # (the generators' own inertias need not meet the triangle inequality: neither do these)


@pytest.mark.parametrize("case", CASES)
def test_own_parameters_equal_the_plain_oracle_exactly(case):
    """(a) every row with the description's own numbers: bit for bit OracleModel(desc)."""
    sys_, desc = make_case(case)
    q, qd, qdd, tau, _ = batch(sys_, desc, 4)
    own = np.broadcast_to(ipc.parameters_of(desc), (4, desc.n_joints, 10))
    om, ck = OracleModel(desc), ipc.Checker(desc)
    # (the symmetric part of J: the lumped body's J is symmetric up to the rounding of its congruences, parameter_vector reads its upper half)
    assert np.abs(ipc.parameters_of(desc).reshape(-1) - om.parameter_vector()).max() <= 1e-15 * np.abs(om.parameter_vector()).max()
    assert np.array_equal(ck.rnea(q, qd, qdd, own, GRAVITY), om.rnea(q, qd, qdd, GRAVITY))
    assert np.array_equal(ck.aba(q, qd, tau, own, GRAVITY), om.aba(q, qd, tau, GRAVITY))
    assert len(ck._models) == 1  # cached per distinct parameter set


@pytest.mark.parametrize("case", CASES)
def test_tau_is_regressor_times_first_moment_parameters(case):
    """(b) tau of row r = Y(q, qd, qdd) (m, m c, J) of row r, to 1e-10 max(1, |tau|)."""
    sys_, desc = make_case(case)
    B = 3
    q, qd, qdd, _, pi = batch(sys_, desc, B)
    tau = ipc.Checker(desc).rnea(q, qd, qdd, pi, GRAVITY)
    Y = ipc.first_moment_regressor(desc, q, qd, qdd, GRAVITY)
    lin = ipc.first_moment_form(pi).reshape(B, -1)
    ref = np.einsum("bij,bj->bi", Y, lin)
    err, bound = np.abs(tau - ref).max(), 1e-10 * max(1.0, np.abs(tau).max())
    print(f"{case}: |tau - Y pi|_inf = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("case", CASES)
def test_forward_dynamics_inverts_inverse_dynamics_per_row(case):
    """(c) aba(rnea(qdd)) = qdd on every row, within helpers.close_aba's per-row bound (cond_inf of the row's own H)."""
    sys_, desc = make_case(case)
    B = 6
    q, qd, qdd, _, pi = batch(sys_, desc, B)
    f = np.random.default_rng(9).uniform(-5.0, 5.0, (B, desc.n_joints, 6))
    ck = ipc.Checker(desc)
    tau = ck.rnea(q, qd, qdd, pi, GRAVITY, f)
    back = ck.aba(q, qd, tau, pi, GRAVITY, f)
    ratio = close_aba(back, qdd, ck.crba(q, pi), desc.n_joints, label=f"{case}: aba(rnea(qdd))")
    print(f"{case}: worst err / (cond u) = {ratio:.3e}")


@pytest.mark.parametrize("case", CASES)
def test_doubling_a_rows_parameters_doubles_its_efforts(case):
    """(d) (m, c, J) -> (2 m, c, 2 J) is what doubling every inertia does; the issue's pin doubles every NUMBER of the row, com included:
    tau is linear in (m, m c, J), so (2 m, 2 c, 2 J) gives (2 m, 4 m c, 2 J) -- twice tau only where c = 0.  Both readings are checked:
    the literal one on the rows whose bodies have c = 0, the physical one (twice the inertia, same place) on all of them."""
    sys_, desc = make_case(case)
    B = 4
    q, qd, qdd, _, pi = batch(sys_, desc, B)
    ck = ipc.Checker(desc)
    tau = ck.rnea(q, qd, qdd, pi, GRAVITY)
    twice = pi.copy()
    twice[..., 0] *= 2.0
    twice[..., 4:] *= 2.0
    assert np.abs(ck.rnea(q, qd, qdd, twice, GRAVITY) - 2.0 * tau).max() <= 1e-12 * max(1.0, np.abs(tau).max())
    centred = pi.copy()
    centred[..., 1:4] = 0.0
    tau0 = ck.rnea(q, qd, qdd, centred, GRAVITY)
    assert np.abs(ck.rnea(q, qd, qdd, 2.0 * centred, GRAVITY) - 2.0 * tau0).max() <= 1e-12 * max(1.0, np.abs(tau0).max())


@pytest.mark.parametrize("case", CASES)
def test_coriolis_switch_of_the_checker_is_zero_velocity(case):
    """The checker evaluates consider_coriolis=False as qd = 0 (see Checker.rnea).  Where no centre of mass is off its origin that is
    bit for bit the oracle's own switch; with offsets the oracle's switch differs by the reference's unscaled c x a, visibly."""
    sys_, desc = make_case(case)
    B = 4
    q, qd, qdd, _, pi = batch(sys_, desc, B)
    ck = ipc.Checker(desc)
    centred = pi.copy()
    centred[..., 1:4] = 0.0
    own_switch = np.stack([ck.model(centred[r]).rnea(q[r:r + 1], qd[r:r + 1], qdd[r:r + 1], GRAVITY, None, False, True)[0] for r in range(B)])
    assert np.array_equal(ck.rnea(q, qd, qdd, centred, GRAVITY, None, False, True), own_switch)
    quirk = np.stack([ck.model(pi[r]).rnea(q[r:r + 1], qd[r:r + 1], qdd[r:r + 1], GRAVITY, None, False, True)[0] for r in range(B)])
    assert np.abs(ck.rnea(q, qd, qdd, pi, GRAVITY, None, False, True) - quirk).max() > 1e-3
