"""Pins of the CPU checker of the step linearisation (tests/step_derivatives_check.py) and of the names of the six exports on the host
side.  No GPU: the checker is numpy; the references are the C oracle's state integrator and central differences of the oracle's own step
(OracleModel.aba, then OracleModel.integrate)."""
import os
import re

import numpy as np
import pytest

import dynamics_derivatives_check as dc
import gravity_gradient_check as gc
import step_derivatives_check as sc
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mh_configuration_add_f64", "mh_configuration_add_f32", "mh_configuration_difference_f64", "mh_configuration_difference_f32",
         "mh_aba_integrate_derivatives_f64", "mh_aba_integrate_derivatives_f32")


def state(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)


@pytest.mark.parametrize("case", CASES)
def test_add_and_difference_invert_each_other(case):
    sys_, desc = make_case(case)
    m, B = sc.StepModel(desc), 6
    q0, q1 = state(sys_, B, 5)[0], state(sys_, B, 6)[0]
    rng = np.random.default_rng(2)
    dq = rng.uniform(-1.0, 1.0, (B, desc.nv))  # (|dth| <= sqrt(3) < pi)
    dq[0] *= 1.0e-9
    back = sc.configuration_difference(m, q0, sc.configuration_add(m, q0, dq))
    assert np.abs(back - dq).max() <= 1.0e-12
    d = sc.configuration_difference(m, q0, q1)
    q1n = sc.configuration_add(m, q0, d)
    for b in range(B):  # q1 up to the sign and the norm of its quaternions: the same poses
        assert np.abs(sc.configuration_difference_one(m, q1[b], q1n[b])).max() <= 1.0e-12
        R0, p0 = m.world_poses(q1[b])[:2]
        R1, p1 = m.world_poses(q1n[b])[:2]
        assert max(np.abs(np.asarray(R0) - np.asarray(R1)).max(), np.abs(np.asarray(p0) - np.asarray(p1)).max()) <= 1.0e-12


@pytest.mark.parametrize("case", CASES)
def test_add_of_a_single_dof_is_the_oracles_integrator(case):
    """With dq non-zero in one DoF the double integrator's w x v term vanishes: OracleModel.integrate(1, q, dq, 0) is q (+) dq."""
    sys_, desc = make_case(case)
    m, om = sc.StepModel(desc), OracleModel(desc)
    q = state(sys_, 3)[0]
    z = np.zeros((3, desc.nv))
    for k in range(desc.nv):
        dq = z.copy()
        dq[:, k] = [0.7, -1.3, 1.0e-9]
        assert np.abs(sc.configuration_add(m, q, dq) - om.integrate(1.0, q, dq, z)[0]).max() <= 1.0e-14


def oracle_step(om, dt, q, qd, tau, f):
    qdd = om.aba(q[None], qd[None], tau[None], GRAVITY, None if f is None else f[None])
    qn, vn, _ = om.integrate(dt, q[None], qd[None], qdd)
    return qn[0], vn[0]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dt", [0.1, 1.0e-3])
def test_columns_against_central_differences_of_the_oracles_step(case, dt):
    """Every column of A and B against a central difference (h = 1e-5) of the oracle's step: inputs stepped through (+) with the wrenches
    held in the world, outputs differenced through (-) from the unperturbed new configuration.  Bound: test_forward_dynamics_derivatives'
    form, 2e-5 cond_inf(H) max(1, |matrix|_inf).  Worst error / bound, dt = 0.1 | 1e-3: arm7 3.2e-8 | 5.0e-9, humanoid30 1.4e-8 | 1.1e-9,
    onedof_tree 8.4e-9 | 5.9e-9, planar 5.6e-8 | 2.3e-8, spherical 3.0e-8 | 1.3e-8, fixed 6.7e-8 | 3.6e-8, lumped 7.4e-8 | 2.8e-8."""
    sys_, desc = make_case(case)
    om, m, B, h = OracleModel(desc), sc.StepModel(desc), 2, 1.0e-5
    q, qd, _, tau = state(sys_, B)
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    H = om.crba(q)
    nv, worst = m.nv, 0.0
    for b in range(B):
        fb = f[b] if b == 0 else None
        _, A, Bm, _, _ = sc.step_derivatives_one(m, dt, q[b], qd[b], tau[b], GRAVITY, fb)
        cond = np.linalg.cond(H[b], np.inf)
        q_new = oracle_step(om, dt, q[b], qd[b], tau[b], fb)[0]
        owned = np.zeros(nv, dtype=bool)
        owned[np.concatenate([m.dofs(i) for i in range(m.n)])] = True

        def column(which, k):
            out = []
            for s in (h, -h):
                e = np.zeros(nv)
                e[k] = s
                q1, qd1, tau1, f1 = q[b], qd[b], tau[b], fb
                if which == 0:
                    q1 = sc.configuration_add_one(m, q[b], e)
                    f1 = None if fb is None else gc.wrenches_held_in_world(m, q[b], q1, fb)
                elif which == 1:
                    qd1 = qd[b] + e
                else:
                    tau1 = tau[b] + e
                qn, vn = oracle_step(om, dt, q1, qd1, tau1, f1)
                out.append(np.concatenate([sc.configuration_difference_one(m, q_new, qn), vn]))
            return (out[0] - out[1]) / (2.0 * h)

        for k in np.flatnonzero(owned):
            ea = max(np.abs(column(0, k) - A[:, k]).max(), np.abs(column(1, k) - A[:, nv + k]).max())
            eb = np.abs(column(2, k) - Bm[:, k]).max()
            worst = max(worst, ea / (2.0e-5 * cond * max(1.0, np.abs(A).max())), eb / (2.0e-5 * cond * max(1.0, np.abs(Bm).max())))
    print(f"{case} dt {dt}: worst err / bound {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", CASES)
def test_zero_step_is_the_identity(case):
    sys_, desc = make_case(case)
    m = sc.StepModel(desc)
    q, qd, _, tau = state(sys_, 1)
    _, A, Bm, Aa, Ba = sc.step_derivatives_one(m, 0.0, q[0], qd[0], tau[0], GRAVITY)
    owned = np.zeros(2 * m.nv)
    for i in range(m.n):
        owned[m.dofs(i)] = owned[m.nv + m.dofs(i)] = 1.0
    assert np.array_equal(A, np.diag(owned)) and not Bm.any()
    assert np.all(Aa >= np.abs(A)) and np.all(Ba >= np.abs(Bm))


@pytest.mark.parametrize("case", ["humanoid30", "spherical", "planar"])
def test_small_angle_branch_is_continuous(case):
    """qd = 0 and the tau that holds the robot (qdd = 0) give r = 0, the branch below the step's threshold; a state whose rotation vectors
    are 1e-9 long gives the same matrices to 1e-8."""
    sys_, desc = make_case(case)
    m, om, dt = sc.StepModel(desc), OracleModel(desc), 0.1
    q = state(sys_, 1)[0]
    z = np.zeros((1, desc.nv))
    tau = om.rnea(q, z, z, GRAVITY, None, True, True)
    qdd, Dq, Dv, Hinv = dc.aba_derivatives_one(m, q[0], z[0], tau[0], GRAVITY)
    assert np.abs(qdd).max() <= 1.0e-9
    A0, B0, _, _ = sc.assemble_one(m, dt, z[0], z[0], Dq, Dv, Hinv)
    A1, B1, _, _ = sc.assemble_one(m, dt, np.full(desc.nv, 1.0e-9 / dt), z[0], Dq, Dv, Hinv)
    assert np.abs(A1 - A0).max() <= 1.0e-8 and np.abs(B1 - B0).max() <= 1.0e-8
    assert np.abs(A1 - A0).max() > 0.0


def test_abs_sums_dominate():
    sys_, desc = make_case("humanoid30")
    m = sc.StepModel(desc)
    q, qd, _, tau = state(sys_, 1)
    _, A, Bm, Aa, Ba = sc.step_derivatives_one(m, 0.1, q[0], qd[0], tau[0], GRAVITY)
    assert np.all(Aa >= np.abs(A) * (1.0 - 1e-12)) and np.all(Ba >= np.abs(Bm) * (1.0 - 1e-12))


def test_exports_are_named_on_every_host_side():
    """include/mecano_hip.h, the ctypes symbol list, the Panama binding and INTEGRATION.md all carry the six exports."""
    from mecano_amd import _lib
    header = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
    native = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\bmh_status\s+%s\s*\(" % name, header), name
        assert name in _lib.ABI_SYMBOLS, name
        assert re.search(r'handle\(\s*"%s"' % name, native), name
        assert name[:-4] in guide, name
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", header)  # purely additive
