"""Pins of the CPU checker of the state-and-parameter gradient calls (tests/parameters_state_vjp_check.py): at the model's own
parameters it is the shared-parameter checker, and at per-row parameters its state gradients are central differences of the per-row
oracle (inertial_parameters_check.Checker) along random directions.  No GPU."""
import numpy as np
import pytest

import dynamics_vjp_check as vc
import inertial_parameters_check as ipc
import parameters_state_vjp_check as sc
import parameters_vjp_check as pc
from mecano_amd import random_tools as rt
from test_gravity_gradient_cpu import GRAVITY, make_case, random_wrenches

ROWS = 3
H_STEP = 1.0e-5   # the step of test_dynamics_derivatives_cpu.py::test_columns_against_finite_differences_of_the_oracle and of
FD_TOL = 2.0e-5   # test_dynamics_vjp_cpu.py::test_chart_pullback_against_raw_finite_differences, and their bound per gradient entry


def case(name):
    return sc.floating_tree7() if name == "n3_floating_tree7" else make_case(name)


def inputs(name):
    sys_, desc = case(name)
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(5), sys_, ROWS)
    u = np.random.default_rng(8).uniform(-1.0, 1.0, (ROWS, desc.nv))
    return sys_, desc, q, qd, qdd, tau, u


@pytest.mark.parametrize("name", ["arm7", "humanoid30", "lumped"])
def test_own_parameters_give_the_shared_parameter_checker(name):
    """Every row at inertial_parameters(): the state gradients are dynamics_vjp_check on the description itself, bit for bit, and gpi
    is parameters_vjp_check's.  arm7 also through desc_with(own numbers): the same gradients to 1e-12 (the description rebuilt from ten
    numbers)."""
    sys_, desc, q, qd, qdd, tau, u = inputs(name)
    f = random_wrenches(np.random.default_rng(3), ROWS, desc.n_joints, always=True)
    own = np.broadcast_to(ipc.parameters_of(desc), (ROWS, desc.n_joints, 10)).copy()
    gq, gqd, gqdd, gpi, scales = sc.rnea_parameters_state_vjp(desc, q, qd, qdd, own, u, GRAVITY, f)
    rq, rv, ra, rs = vc.rnea_vjp(desc, q, qd, qdd, u, GRAVITY, f)
    assert np.array_equal(gq, rq) and np.array_equal(gqd, rv) and np.array_equal(gqdd, ra)
    assert all(np.array_equal(a, b) for a, b in zip(scales[:3], rs))
    assert np.array_equal(gpi, pc.rnea_parameters_vjp(desc, q, qd, qdd, own, u, GRAVITY)[0])
    qdd_f, fq, fv, ft, fpi, fscales = sc.aba_parameters_state_vjp(desc, q, qd, tau, own, u, GRAVITY, f)
    ref = vc.aba_vjp(desc, q, qd, tau, u, GRAVITY, f)
    assert all(np.array_equal(a, b) for a, b in zip((qdd_f, fq, fv, ft), ref[:4]))
    assert np.array_equal(fpi, pc.aba_parameters_vjp(desc, q, qd, tau, own, u, GRAVITY, f)[2])
    assert np.all(fscales[5] >= 1.0) and np.all(scales[5] >= 1.0)
    if name == "arm7":
        rebuilt = ipc.desc_with(desc, own[0])
        for a, b in zip(vc.rnea_vjp(rebuilt, q, qd, qdd, u, GRAVITY, f)[:3], (rq, rv, ra)):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def _central(fn, om, q, qd, x3, dq, dqd, dx3):
    """Central differences of fn(q, qd, x3) [1, nv] with step H_STEP: along the integrator's step of velocity dq (the chart of
    tests/dynamics_derivatives_check.py: fd_columns of test_dynamics_derivatives_cpu.py takes it in one DoF at a time), plain in qd, x3."""
    z = np.zeros_like(qd)
    out = []
    for a, b, c in ((dq, None, None), (None, dqd, None), (None, None, dx3)):
        vals = []
        for step in (H_STEP, -H_STEP):
            q1 = q if a is None else om.integrate(step, q, a, z)[0]
            vals.append(fn(q1, qd if b is None else qd + step * b, x3 if c is None else x3 + step * c)[0])
        out.append((vals[0] - vals[1]) / (2.0 * H_STEP))
    return out


@pytest.mark.parametrize("name", ["arm7", "n3_floating_tree7"])
def test_state_gradients_against_central_differences_of_the_per_row_oracle(name):
    """Rows of physical_parameter_sets.  For random directions d with |d|_inf <= 1: gq . d, gqd . d, g3 . d against the central difference
    of u . Checker.rnea and w . Checker.aba of the row's own model along d.  Bound: the per-entry bound of the shared-parameter
    comparisons, 2e-5 max(1, |g|_inf), summed over the entries the direction weighs: times |d|_1."""
    sys_, desc, q, qd, qdd, tau, u = inputs(name)
    rng = np.random.default_rng(12)
    pi = ipc.physical_parameter_sets(desc, np.random.default_rng(4), ROWS)
    ck = ipc.Checker(desc)
    d = rng.uniform(-1.0, 1.0, (3, ROWS, desc.nv))
    gq, gqd, gqdd, _, _ = sc.rnea_parameters_state_vjp(desc, q, qd, qdd, pi, u, GRAVITY)
    _, fq, fv, ft, _, _ = sc.aba_parameters_state_vjp(desc, q, qd, tau, pi, u, GRAVITY)
    assert np.abs(gq[0] - gq[1]).max() > 1e-3  # (rows differ)
    worst = 0.0
    for r in range(ROWS):
        om = ck.model(pi[r])
        s = slice(r, r + 1)
        inv = lambda q_, qd_, x_: om.rnea(q_, qd_, x_, GRAVITY, None)
        fwd = lambda q_, qd_, x_: om.aba(q_, qd_, x_, GRAVITY, None)
        for fn, x3, grads in ((inv, qdd, (gq, gqd, gqdd)), (fwd, tau, (fq, fv, ft))):
            fd = _central(fn, om, q[s], qd[s], x3[s], d[0, s], d[1, s], d[2, s])
            for k, (g, col) in enumerate(zip(grads, fd)):
                got, ref = float(g[r] @ d[k, r]), float(u[r] @ col)
                bound = FD_TOL * max(1.0, np.abs(g[r]).max()) * np.abs(d[k, r]).sum()
                worst = max(worst, abs(got - ref) / bound)
                assert abs(got - ref) <= bound, (name, r, fn is fwd, k, got, ref, bound)
    print(f"{name}: directional derivatives against central differences, worst achieved / bound {worst:.3e}")


def test_rows_argument_leaves_the_other_rows_zero():
    sys_, desc, q, qd, qdd, tau, u = inputs("arm7")
    pi = ipc.physical_parameter_sets(desc, np.random.default_rng(4), ROWS)
    full = sc.rnea_parameters_state_vjp(desc, q, qd, qdd, pi, u, GRAVITY)
    part = sc.rnea_parameters_state_vjp(desc, q, qd, qdd, pi, u, GRAVITY, rows=[1])
    for a, b in zip(full[:4], part[:4]):
        assert np.array_equal(a[1], b[1]) and not b[0].any() and not b[2].any()
