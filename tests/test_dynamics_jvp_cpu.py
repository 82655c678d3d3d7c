"""Pins of the CPU side of the forward-mode calls: the checker's contraction (tests/dynamics_jvp_check.py) against the O(n) recursion
the device kernel is built on, against the reverse-mode checkers by duality, and against central differences of the C oracle's inverse
and forward dynamics along the directions.  No GPU."""
import numpy as np
import pytest

import dynamics_derivatives_check as dc
import dynamics_jvp_check as jc
import dynamics_vjp_check as vc
import gravity_gradient_check as gc
import step_derivatives_check as sc
import step_vjp_check as svc
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel
from test_dynamics_vjp_cpu import ROOT_ACC, floating_mixed
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

DT = 0.01


def case_of(case):
    return floating_mixed() if case == "floating_mixed" else make_case(case)


def directions(desc, B, seed=8):
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(-1.0, 1.0, (B, desc.nv)) for _ in range(3))


@pytest.mark.parametrize("case", CASES + ["floating_mixed"])
@pytest.mark.parametrize("gravity", [GRAVITY, ROOT_ACC], ids=["gravity", "root_acceleration"])
def test_sweeps_equal_the_contraction(case, gravity):
    """The two-sweep tangent recursion against D dq + D' dqd + H dqdd of the checker's matrices, and its tau_in form against
    tau_in - (.): 1e-11 relative to max(1, |.|_inf) -- both sides are the same sums in another order."""
    sys_, desc = case_of(case)
    m, B = dc.DerivativeModel(desc), 3
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(5), sys_, B)
    dq, dqd, dqdd = directions(desc, B)
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    f[1] = 0.0
    ref, _ = jc.rnea_jvp(desc, q, qd, qdd, dq, dqd, dqdd, gravity, f)
    ref0, _ = jc.rnea_jvp(desc, q, qd, qdd, dq, dqd, None, gravity, f)
    own = jc.owned(m)
    worst = 0.0
    for b in range(B):
        fb = f[b] if b != 1 else None
        got = jc.rnea_jvp_sweeps_one(m, q[b], qd[b], qdd[b], dq[b], dqd[b], dqdd[b], gravity, fb)
        rhs = jc.rnea_jvp_sweeps_one(m, q[b], qd[b], qdd[b], dq[b], dqd[b], np.zeros(desc.nv), gravity, fb, tau_in=tau[b])
        for g, r in ((got, ref[b]), (rhs, np.where(own, tau[b] - ref0[b], 0.0))):
            worst = max(worst, float(np.abs(g - r).max()) / max(1.0, float(np.abs(r).max())))
    print(f"{case}: sweeps against the contraction, worst relative error {worst:.3e}")
    assert worst <= 1.0e-11


def test_zero_directions_give_exact_zeros():
    sys_, desc = make_case("humanoid30")
    m = dc.DerivativeModel(desc)
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(5), sys_, 1)
    z = np.zeros(desc.nv)
    f = random_wrenches(np.random.default_rng(4), 1, desc.n_joints, always=True)
    assert np.all(jc.rnea_jvp_sweeps_one(m, q[0], qd[0], qdd[0], z, z, z, GRAVITY, f[0]) == 0.0)
    Z = np.zeros((1, desc.nv))
    assert np.all(jc.rnea_jvp(desc, q, qd, qdd, Z, Z, Z, GRAVITY, f)[0] == 0.0)
    assert np.all(jc.aba_jvp(desc, q, qd, tau, Z, Z, Z, GRAVITY, f)[1] == 0.0)
    a, b, _ = jc.integrate_jvp(desc, DT, qd, qdd, Z, Z, Z)
    assert np.all(a == 0.0) and np.all(b == 0.0)
    out = jc.step_jvp(desc, DT, q, qd, tau, Z, Z, Z, GRAVITY, f)
    assert all(np.all(x == 0.0) for x in out[1:4])
    # without velocities dqd has no effect on the efforts
    dqd = directions(desc, 1)[1]
    assert np.all(jc.rnea_jvp_sweeps_one(m, q[0], z, qdd[0], z, dqd[0], z, GRAVITY) == 0.0)


@pytest.mark.parametrize("case", ["floating_mixed", "humanoid30", "planar", "spherical"])
def test_duality_with_the_reverse_mode_checkers(case):
    """u . J d = (J^T u) . d for every call: 1e-12 relative to the size of the terms for the inverse dynamics and the integrator, times
    cond_inf(H) for the forward forms (both checkers go through H^-1)."""
    sys_, desc = case_of(case)
    B = 2
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(5), sys_, B)
    dq, dqd, d3 = directions(desc, B)
    u, u2 = directions(desc, B, seed=9)[:2]
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    cond = float(np.linalg.cond(OracleModel(desc).crba(q), np.inf).max())
    dot = lambda a, b: np.einsum("bi,bi->b", a, b)
    size = lambda *pairs: np.maximum(1.0, sum(np.einsum("bi,bi->b", np.abs(a), np.abs(b)) for a, b in pairs))

    dtau, _ = jc.rnea_jvp(desc, q, qd, qdd, dq, dqd, d3, GRAVITY, f)
    gq, gqd, gqdd, _ = vc.rnea_vjp(desc, q, qd, qdd, u, GRAVITY, f)
    e_rnea = np.abs(dot(u, dtau) - dot(gq, dq) - dot(gqd, dqd) - dot(gqdd, d3)) / size((u, dtau), (gq, dq), (gqd, dqd), (gqdd, d3))

    _, dqdd, _ = jc.aba_jvp(desc, q, qd, tau, dq, dqd, d3, GRAVITY, f)
    _, gq, gqd, gtau, _ = vc.aba_vjp(desc, q, qd, tau, u, GRAVITY, f)
    e_aba = np.abs(dot(u, dqdd) - dot(gq, dq) - dot(gqd, dqd) - dot(gtau, d3)) / size((u, dqdd), (gq, dq), (gqd, dqd), (gtau, d3))

    dqn, dqdn, _ = jc.integrate_jvp(desc, DT, qd, qdd, dq, dqd, d3)
    gq, gqd, gqdd, _ = svc.integrate_vjp(desc, DT, qd, qdd, u, u2)
    e_int = np.abs(dot(u, dqn) + dot(u2, dqdn) - dot(gq, dq) - dot(gqd, dqd) - dot(gqdd, d3)) / size((u, dqn), (u2, dqdn), (gq, dq), (gqd, dqd), (gqdd, d3))

    out = jc.step_jvp(desc, DT, q, qd, tau, dq, dqd, d3, GRAVITY, f)
    _, gq, gqd, gtau, _, _ = svc.step_vjp(desc, DT, q, qd, tau, u, u2, GRAVITY, f)
    e_step = np.abs(dot(u, out[2]) + dot(u2, out[3]) - dot(gq, dq) - dot(gqd, dqd) - dot(gtau, d3)) / size((u, out[2]), (u2, out[3]), (gq, dq), (gqd, dqd), (gtau, d3))
    print(f"{case}: duality rnea {e_rnea.max():.3e}, integrate {e_int.max():.3e} (bound 1e-12); aba {e_aba.max():.3e}, step {e_step.max():.3e} "
          f"(bound {1e-12 * cond:.3e})")
    assert e_rnea.max() <= 1.0e-12 and e_int.max() <= 1.0e-12
    assert e_aba.max() <= 1.0e-12 * cond and e_step.max() <= 1.0e-12 * cond
    # the step's dqdd is that of the forward dynamics alone (the same matrices, contracted by another routine)
    assert np.abs(out[1] - dqdd).max() <= 1.0e-12 * max(1.0, float(np.abs(dqdd).max()))


@pytest.mark.parametrize("case", ["floating_mixed", "humanoid30", "planar", "spherical"])
def test_against_central_differences_of_the_oracle(case):
    """rnea(q (+) h dq, qd + h dqd, qdd + h dqdd) and the forward dynamics likewise, by central differences with h = 1e-5 and the wrenches
    held in the world, against the checker's products.  Bound: 2e-5 relative to max(1, |.|_inf), that of
    test_dynamics_derivatives_cpu.py::test_columns_against_finite_differences_of_the_oracle."""
    sys_, desc = case_of(case)
    om, m, B, h = OracleModel(desc), dc.DerivativeModel(desc), 2, 1.0e-5
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(5), sys_, B)
    dq, dqd, d3 = directions(desc, B)
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    f[1] = 0.0
    dtau, _ = jc.rnea_jvp(desc, q, qd, qdd, dq, dqd, d3, GRAVITY, f)
    _, dqdd, _ = jc.aba_jvp(desc, q, qd, tau, dq, dqd, d3, GRAVITY, f)
    fd_tau, fd_qdd = [], []
    for s in (h, -h):
        q1 = sc.configuration_add(m, q, s * dq)
        f1 = np.stack([gc.wrenches_held_in_world(m, q[b], q1[b], f[b]) for b in range(B)])
        fd_tau.append(om.rnea(q1, qd + s * dqd, qdd + s * d3, GRAVITY, f1, True, True))
        fd_qdd.append(om.aba(q1, qd + s * dqd, tau + s * d3, GRAVITY, f1))
    e_tau = float(np.abs((fd_tau[0] - fd_tau[1]) / (2.0 * h) - dtau).max())
    e_qdd = float(np.abs((fd_qdd[0] - fd_qdd[1]) / (2.0 * h) - dqdd).max())
    print(f"{case}: central differences, dtau err {e_tau:.3e} (|.| up to {np.abs(dtau).max():.3g}), dqdd err {e_qdd:.3e} "
          f"(|.| up to {np.abs(dqdd).max():.3g})")
    assert e_tau <= 2.0e-5 * max(1.0, float(np.abs(dtau).max()))
    assert e_qdd <= 2.0e-5 * max(1.0, float(np.abs(dqdd).max()))
