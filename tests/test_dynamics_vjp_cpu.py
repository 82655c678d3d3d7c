"""Pins of the CPU side of the reverse-mode gradient calls: the checker's contraction (tests/dynamics_vjp_check.py) against the O(n)
identities the device kernel is built on, and ``chart_pullback`` against central differences in RAW coordinates of the C oracle's forward
dynamics.  No GPU."""
import numpy as np
import pytest
import torch

import dynamics_derivatives_check as dc
import dynamics_vjp_check as vc
from mecano_amd import autograd as mha
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

ROOT_ACC = np.array([0.4, -0.3, 0.2, 1.5, -0.7, 9.0])


def floating_mixed(seed=7):
    """A SixDoF root with a tree of revolute, spherical, planar and prismatic joints below it."""
    joints = rt.nextFloatingChain(np.random.default_rng(seed), 6, ("revolute", "spherical", "planar", "prismatic"), tree=True)
    sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
    return sys_, sys_.toModelDesc()


@pytest.mark.parametrize("case", CASES + ["floating_mixed"])
@pytest.mark.parametrize("gravity", [GRAVITY, ROOT_ACC], ids=["gravity", "root_acceleration"])
def test_sweeps_equal_the_contraction(case, gravity):
    """The two-sweep form (X1, X4, X5 per body) against u^T D and H u of the checker's matrices: 1e-11 relative to max(1, |.|_inf) -- both
    sides are the same sums in another order."""
    sys_, desc = floating_mixed() if case == "floating_mixed" else make_case(case)
    m, B = dc.DerivativeModel(desc), 3
    q, qd, qdd, _ = rt.nextState(np.random.default_rng(5), sys_, B)
    u = np.random.default_rng(8).uniform(-1.0, 1.0, (B, desc.nv))
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    f[1] = 0.0
    gq, gqd, gqdd, _ = vc.rnea_vjp(desc, q, qd, qdd, u, gravity, f)
    worst = 0.0
    for b in range(B):
        sq, sv, sa = vc.rnea_vjp_sweeps_one(m, q[b], qd[b], qdd[b], u[b], gravity, f[b] if b != 1 else None)
        for got, ref in ((sq, gq[b]), (sv, gqd[b]), (sa, gqdd[b])):
            worst = max(worst, float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())))
    print(f"{case}: sweeps against the contraction, worst relative error {worst:.3e}")
    assert worst <= 1.0e-11


def test_sweeps_give_exact_zeros():
    sys_, desc = make_case("humanoid30")
    m = dc.DerivativeModel(desc)
    q, qd, qdd, _ = rt.nextState(np.random.default_rng(5), sys_, 1)
    z = np.zeros(desc.nv)
    assert all(np.all(g == 0.0) for g in vc.rnea_vjp_sweeps_one(m, q[0], qd[0], qdd[0], z, GRAVITY))
    u = np.random.default_rng(8).uniform(-1.0, 1.0, desc.nv)
    assert np.all(vc.rnea_vjp_sweeps_one(m, q[0], z, qdd[0], u, GRAVITY)[1] == 0.0)


def test_forward_contraction_solves_the_adjoint_system():
    """gtau = H^-1 w, gq = -(d tau / d q)^T gtau, gqd = -(d tau / d qd)^T gtau at qdd = aba: what mh_aba_vjp_* composes."""
    sys_, desc = make_case("humanoid30")
    B = 2
    q, qd, _, tau = rt.nextState(np.random.default_rng(5), sys_, B)
    w = np.random.default_rng(9).uniform(-1.0, 1.0, (B, desc.nv))
    qdd, gq, gqd, gtau, _ = vc.aba_vjp(desc, q, qd, tau, w, GRAVITY)
    rq, rv, ra, _ = vc.rnea_vjp(desc, q, qd, qdd, gtau, GRAVITY)
    cond = np.linalg.cond(OracleModel(desc).crba(q), np.inf).max()
    assert np.abs(ra - w).max() <= 1e-10 * cond
    assert np.abs(rq + gq).max() <= 1e-10 * cond * max(1.0, np.abs(gq).max())
    assert np.abs(rv + gqd).max() <= 1e-10 * cond * max(1.0, np.abs(gqd).max())


@pytest.mark.parametrize("case", ["floating_mixed", "humanoid30", "planar", "spherical"])
def test_chart_pullback_against_raw_finite_differences(case):
    """L(q_raw) = w^T aba(q_raw, qd, tau) of the oracle, differentiated by central differences (h = 1e-5) in every raw coordinate --
    quaternion entries included, with unnormalised quaternions among the inputs -- against chart_pullback of the checker's velocity-space
    gradient.  Bound: 2e-5 relative to max(1, |gradient|_inf), that of
    test_dynamics_derivatives_cpu.py::test_columns_against_finite_differences_of_the_oracle."""
    sys_, desc = floating_mixed() if case == "floating_mixed" else make_case(case)
    if case == "floating_mixed":
        kinds = set(int(t) for t in desc.joint_type)
        assert {mha.SIXDOF, mha.SPHERICAL, mha.PLANAR} <= kinds
    om, B, h = OracleModel(desc), 3, 1.0e-5
    q, qd, _, tau = rt.nextState(np.random.default_rng(5), sys_, B)
    maps = mha.chart_maps(desc)
    scale = np.random.default_rng(2).uniform(0.6, 1.7, (B, len(maps["quat_q"])))
    scale[0] = 1.0  # the first configuration keeps unit quaternions
    for k, rows in enumerate(maps["quat_q"]):
        q[:, rows] *= scale[:, k:k + 1]
    w = np.random.default_rng(9).uniform(-1.0, 1.0, (B, desc.nv))
    loss = lambda q_: np.einsum("bi,bi->b", w, om.aba(q_, qd, tau, GRAVITY, None))
    _, gq, _, _, _ = vc.aba_vjp(desc, q, qd, tau, w, GRAVITY)
    got = mha.chart_pullback(desc, torch.from_numpy(q), torch.from_numpy(gq)).numpy()
    ref = np.zeros_like(q)
    for k in range(desc.nq):
        e = np.zeros_like(q)
        e[:, k] = h
        ref[:, k] = (loss(q + e) - loss(q - e)) / (2.0 * h)
    err = float(np.abs(got - ref).max())
    print(f"{case}: raw-coordinate gradient, max err {err:.3e} (|.| up to {np.abs(ref).max():.3g})")
    assert err <= 2.0e-5 * max(1.0, float(np.abs(ref).max()))
    owned = sorted(set(maps["one_q"]) | {i for r in maps["quat_q"] + maps["lin_q"] + maps["pl_q"] for i in r})
    assert np.all(np.delete(got, owned, axis=1) == 0.0)


def test_chart_pullback_is_orthogonal_to_the_quaternion_and_refuses_wrong_shapes():
    _, desc = floating_mixed()
    rng = np.random.default_rng(1)
    q, g = torch.from_numpy(rng.normal(size=(4, desc.nq))), torch.from_numpy(rng.normal(size=(4, desc.nv)))
    out = mha.chart_pullback(desc, q, g)
    for rows in mha.chart_maps(desc)["quat_q"]:
        assert float((out[:, rows] * q[:, rows]).sum(-1).abs().max()) <= 1e-12
    with pytest.raises(ValueError):
        mha.chart_pullback(desc, q, g[:, :-1])
    with pytest.raises(ValueError):
        mha.chart_pullback(desc, q[:3], g)
