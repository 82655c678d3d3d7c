"""Pins of the CPU checker of the dynamics-derivative calls (tests/dynamics_derivatives_check.py), and of the names of the four exports
on the host side.  No GPU: the checker is numpy; the references are the reference calculator's restatement at rest
(gravity_gradient_check), exact identities of the C oracle's inverse dynamics, and central differences of its inverse and forward
dynamics along its own state integrator."""
import os
import re

import numpy as np
import pytest

import dynamics_derivatives_check as dc
import gravity_gradient_check as gc
from helpers import build_lump_pair
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT_ACC = np.array([0.4, -0.3, 0.2, 1.5, -0.7, 9.0])  # a 6-D root acceleration (angular, linear) in place of gravity


def state(sys_, B, seed=5):
    q, qd, qdd, tau = rt.nextState(np.random.default_rng(seed), sys_, B)
    return q, qd, qdd, tau


def oracle_rnea(om, q, qd, qdd, g, f):
    """The oracle's inverse dynamics with both switches ON (holding_efforts' note: with the Coriolis switch off a body whose centre of
    mass is off its frame's origin -- the lumped model's -- goes down a branch that leaves c x a unscaled; qd = 0 is given as zeros)."""
    return om.rnea(q, qd, qdd, g, f, True, True)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("with_wrenches", [False, True])
def test_at_rest_it_is_the_gravity_gradient(case, with_wrenches):
    sys_, desc = make_case(case)
    B = 4
    q = state(sys_, B)[0]
    z = np.zeros((B, desc.nv))
    f = random_wrenches(np.random.default_rng(3), B, desc.n_joints, always=True) if with_wrenches else None
    tau, dq, dqd = dc.rnea_derivatives(desc, q, z, z, GRAVITY, f)
    tau_ref, grad_ref = gc.gravity_gradient(desc, q, GRAVITY, f)
    e_t, e_g = np.abs(tau - tau_ref).max(), np.abs(dq - grad_ref).max()
    print(f"{case}: tau err {e_t:.3e}, gradient err {e_g:.3e} (|grad| up to {np.abs(grad_ref).max():.3g})")
    assert e_t <= 1.0e-12 * max(1.0, np.abs(tau_ref).max())
    assert e_g <= 1.0e-12 * max(1.0, np.abs(grad_ref).max())
    assert np.all(dqd == 0.0)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gravity", [GRAVITY, ROOT_ACC], ids=["gravity", "root_acceleration"])
def test_velocity_gradient_is_homogeneous_of_degree_two(case, gravity):
    """tau is a quadratic form in qd plus a part without qd, so (d tau / d qd) qd = 2 (rnea(q, qd, qdd) - rnea(q, 0, qdd)) exactly."""
    sys_, desc = make_case(case)
    om, B = OracleModel(desc), 4
    q, qd, qdd, _ = state(sys_, B)
    f = random_wrenches(np.random.default_rng(3), B, desc.n_joints)
    tau, _, dqd = dc.rnea_derivatives(desc, q, qd, qdd, gravity, f)
    t1, t0 = oracle_rnea(om, q, qd, qdd, gravity, f), oracle_rnea(om, q, np.zeros_like(qd), qdd, gravity, f)
    scale = max(1.0, np.abs(t1).max())
    e_tau = np.abs(tau - t1).max()
    e_hom = np.abs(np.einsum("bij,bj->bi", dqd, qd) - 2.0 * (t1 - t0)).max()
    print(f"{case}: tau err {e_tau:.3e}, homogeneity err {e_hom:.3e}")
    assert e_tau <= 1.0e-12 * scale
    assert e_hom <= 1.0e-12 * scale


def fd_columns(om, gm, fn, q, qd, f, k, h):
    """Central differences of fn(q, qd, f) in DoF k: (along the integrator's step of unit velocity in DoF k with the wrenches held in the
    world -- the ORIGINAL qd goes to fn, not the integrator's re-expressed one --, plain in qd_k)."""
    e, z = np.zeros((1, gm.nv)), np.zeros((1, gm.nv))
    e[0, k] = 1.0
    vq, vv = [], []
    for step in (h, -h):
        q1 = om.integrate(step, q[None], e, z)[0]
        f1 = None if f is None else gc.wrenches_held_in_world(gm, q, q1[0], f)[None]
        vq.append(fn(q1, qd[None], f1)[0])
        vv.append(fn(q[None], qd[None] + step * e, None if f is None else f[None])[0])
    return (vq[0] - vq[1]) / (2.0 * h), (vv[0] - vv[1]) / (2.0 * h)


@pytest.mark.parametrize("case", CASES)
def test_columns_against_finite_differences_of_the_oracle(case):
    """Every column of both matrices against a central difference (h = 1e-5) of OracleModel.rnea.  Bound: the reference test's own 2e-5
    (compareAgainstFiniteDifference), relative to max(1, |matrix|_inf).  Achieved by the checker, absolute (d tau / d q, d tau / d qd):
    arm7 8.3e-9 / 7.7e-10, humanoid30 6.2e-8 / 3.4e-9 (entries up to 150 / 47), onedof_tree 1.3e-9 / 4.2e-10, planar 1.2e-9 / 3.1e-10,
    spherical 3.4e-9 / 3.4e-10, fixed 1.7e-9 / 6.1e-10, lumped 7.8e-10 / 4.2e-10."""
    sys_, desc = make_case(case)
    om, m, B = OracleModel(desc), dc.DerivativeModel(desc), 2
    q, qd, qdd, _ = state(sys_, B)
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    f[1] = 0.0  # the second configuration carries none
    _, dq, dqd = dc.rnea_derivatives(m, q, qd, qdd, GRAVITY, f)
    wq = wv = 0.0
    for b in range(B):
        fn = lambda q_, qd_, f_: oracle_rnea(om, q_, qd_, qdd[b][None], GRAVITY, f_)
        for k in range(m.nv):
            cq, cv = fd_columns(om, m, fn, q[b], qd[b], f[b] if b == 0 else None, k, 1.0e-5)
            wq = max(wq, float(np.abs(cq - dq[b][:, k]).max()))
            wv = max(wv, float(np.abs(cv - dqd[b][:, k]).max()))
    print(f"{case}: finite-difference max err dq {wq:.3e} (|.| up to {np.abs(dq).max():.3g}), dqd {wv:.3e} (|.| up to {np.abs(dqd).max():.3g})")
    assert wq <= 2.0e-5 * max(1.0, np.abs(dq).max())
    assert wv <= 2.0e-5 * max(1.0, np.abs(dqd).max())


@pytest.mark.parametrize("case", CASES)
def test_switches(case):
    sys_, desc = make_case(case)
    B = 3
    q, qd, qdd, _ = state(sys_, B)
    z = np.zeros_like(qd)
    f = random_wrenches(np.random.default_rng(6), B, desc.n_joints, always=True)
    off = dc.rnea_derivatives(desc, q, qd, qdd, GRAVITY, f, consider_coriolis=False)
    ref = dc.rnea_derivatives(desc, q, z, qdd, GRAVITY, f)
    assert all(np.array_equal(a, b) for a, b in zip(off, ref))
    assert np.all(off[2] == 0.0)
    off = dc.rnea_derivatives(desc, q, qd, qdd, GRAVITY, f, consider_accelerations=False)
    ref = dc.rnea_derivatives(desc, q, qd, z, GRAVITY, f)
    assert all(np.array_equal(a, b) for a, b in zip(off, ref))
    off = dc.rnea_derivatives(desc, q, qd, None, GRAVITY, f)  # no accelerations given at all
    assert all(np.array_equal(a, b) for a, b in zip(off, ref))


@pytest.mark.parametrize("case", CASES)
def test_unrelated_pairs_are_exactly_zero(case):
    sys_, desc = make_case(case)
    q, qd, qdd, _ = state(sys_, 3)
    f = random_wrenches(np.random.default_rng(6), 3, desc.n_joints, always=True)
    _, dq, dqd = dc.rnea_derivatives(desc, q, qd, qdd, GRAVITY, f)
    rel = gc.related(desc)
    assert np.all(dq[:, ~rel] == 0.0) and np.all(dqd[:, ~rel] == 0.0)
    if case in ("humanoid30", "onedof_tree"):
        assert (~rel).any()
    assert np.abs(dq).max() > 0.0 and np.abs(dqd).max() > 0.0


def test_lumped_subtree_equals_welded_subtree():
    _, lumped = make_case("lumped")
    root, _ = build_lump_pair(weld=True)
    welded = MultiBodySystem.toMultiBodySystemInput(root).toModelDesc()
    rng = np.random.default_rng(2)
    q, qd, qdd = rng.uniform(-1.0, 1.0, (4, lumped.nq)), rng.uniform(-1.0, 1.0, (4, lumped.nv)), rng.uniform(-1.0, 1.0, (4, lumped.nv))
    a = dc.rnea_derivatives(lumped, q, qd, qdd, GRAVITY, None)
    b = dc.rnea_derivatives(welded, q, qd, qdd, GRAVITY, None)
    for x, y in zip(a, b):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())


@pytest.mark.parametrize("case", CASES)
def test_forward_dynamics_derivatives(case):
    """With H and qdd from the oracle the checker's matrices satisfy H D + d tau / d(.) = 0 (1e-10), and they agree with a central
    difference of OracleModel.aba in the form of the inverse-dynamics pin, the bound multiplied by cond_inf(H) of the configuration.
    Achieved, as a fraction of that bound at worst: arm7 8.7e-8, humanoid30 1.4e-8, onedof_tree 1.5e-8, planar 2.0e-7, spherical
    7.3e-8, fixed 2.5e-7, lumped 3.1e-7."""
    sys_, desc = make_case(case)
    om, m, B = OracleModel(desc), dc.DerivativeModel(desc), 2
    q, qd, _, tau = state(sys_, B)
    f = random_wrenches(np.random.default_rng(4), B, desc.n_joints, always=True)
    f[1] = 0.0
    H, qdd = om.crba(q), om.aba(q, qd, tau, GRAVITY, f)
    worst = 0.0
    for b in range(B):
        fb = f[b] if b == 0 else None
        qdd_c, Dq, Dv, Hinv = dc.aba_derivatives_one(m, q[b], qd[b], tau[b], GRAVITY, fb)
        assert np.abs(qdd_c - qdd[b]).max() <= 1e-10 * np.linalg.cond(H[b], np.inf) * max(1.0, np.abs(qdd[b]).max())
        assert np.abs(Hinv @ H[b] - np.eye(m.nv)).max() <= 1e-10 * np.linalg.cond(H[b], np.inf)
        _, Dq, Dv, _ = dc.aba_derivatives_one(m, q[b], qd[b], tau[b], GRAVITY, fb, H=H[b], qdd=qdd[b])
        _, dq, dqd = dc.rnea_derivatives_one(m, q[b], qd[b], qdd[b], GRAVITY, fb)
        assert np.abs(H[b] @ Dq + dq).max() <= 1e-10 * max(1.0, np.abs(dq).max())
        assert np.abs(H[b] @ Dv + dqd).max() <= 1e-10 * max(1.0, np.abs(dqd).max())
        cond = np.linalg.cond(H[b], np.inf)
        fn = lambda q_, qd_, f_: om.aba(q_, qd_, tau[b][None], GRAVITY, f_)
        for k in range(m.nv):
            cq, cv = fd_columns(om, m, fn, q[b], qd[b], fb, k, 1.0e-5)
            eq = float(np.abs(cq - Dq[:, k]).max()) / (2.0e-5 * cond * max(1.0, np.abs(Dq).max()))
            ev = float(np.abs(cv - Dv[:, k]).max()) / (2.0e-5 * cond * max(1.0, np.abs(Dv).max()))
            worst = max(worst, eq, ev)
    print(f"{case}: forward-dynamics finite difference, worst err / bound {worst:.3e}")
    assert worst <= 1.0


def test_exports_are_named_on_every_host_side():
    """include/mecano_hip.h, the ctypes symbol list and the Panama binding all carry the four exports."""
    from mecano_amd import _lib
    header = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
    native = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
    for name in ("mh_rnea_derivatives_f64", "mh_rnea_derivatives_f32", "mh_aba_derivatives_f64", "mh_aba_derivatives_f32"):
        assert re.search(r"\bmh_status\s+%s\s*\(" % name, header), name
        assert name in _lib.ABI_SYMBOLS, name
        assert re.search(r'handle\(\s*"%s"' % name, native), name
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", header)  # purely additive
