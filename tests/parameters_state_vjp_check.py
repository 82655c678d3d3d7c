"""CPU checker of mh_rnea_parameters_state_vjp_* / mh_aba_parameters_state_vjp_*: the gradients of the inverse and the forward dynamics
with respect to the state AND to the ten inertial numbers per body, every row at its own parameters.  TEST INFRASTRUCTURE ONLY -- numpy,
one configuration at a time.

Row r's state gradients are tests/dynamics_vjp_check.py (the matrices of tests/dynamics_derivatives_check.py contracted with the
cotangent, H from the C oracle) on the description with the inertia of every body replaced by pi[r]
(inertial_parameters_check.desc_with); row r's parameter gradient is tests/parameters_vjp_check.py (the oracle's regressor contracted and
chained to (m, c, J)).  Nothing of the device's sweeps is used.  tests/test_parameters_state_vjp_cpu.py pins the state gradients by
central differences of inertial_parameters_check.Checker."""
import numpy as np

import dynamics_vjp_check as vc
import inertial_parameters_check as ipc
import parameters_vjp_check as pc
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem
from oracle.cpu_oracle import OracleModel


def floating_tree7():
    """(system, desc) of the model of tests/golden/n3_floating_tree7.json (tests/golden/make_n3_fixtures.py builds it this way): a SixDoF
    root with a tree of six revolute and prismatic joints below it."""
    joints = rt.nextFloatingChain(np.random.default_rng(1002), 6, ("revolute", "prismatic"), tree=True)
    sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
    return sys_, sys_.toModelDesc()


def _groups(desc, pi, at):
    """[(description, rows)]: the rows `at` grouped by their parameter set, each with the description they are evaluated on -- the
    description itself for its own numbers (a lumped body's J is symmetric only up to rounding, and ten numbers cannot carry its skew
    part: inertial_parameters_check.Checker.model does the same), inertial_parameters_check.desc_with(desc, pi[r]) otherwise."""
    own = ipc.parameters_of(desc)
    by_set = {}
    for r in at:
        by_set.setdefault(pi[r].tobytes(), []).append(int(r))
    return [(desc if np.array_equal(pi[rows[0]], own) else ipc.desc_with(desc, pi[rows[0]]), np.array(rows)) for rows in by_set.values()]


def _rows(B, rows):
    return np.arange(B) if rows is None else np.asarray(rows)


def rnea_parameters_state_vjp(desc, q, qd, qdd, pi, u, gravity, f_ext=None, consider_coriolis=True, consider_accelerations=True, rows=None):
    """(gq, gqd, gqdd [B, nv], gpi [B, n, 10], scales): scales = (|d tau / d q|_inf, |d tau / d qd|_inf, |H|_inf, |Y|_inf, chi,
    cond_inf(H(pi_r))), [B] each -- what the bounds of the GPU tests scale with.  rows: the rows to evaluate; the others stay zero (their
    scales one)."""
    B, n, nv = q.shape[0], desc.n_joints, desc.nv
    pi = np.ascontiguousarray(pi, dtype=np.float64).reshape(B, n, 10)
    gq, gqd, gqdd = np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv))
    sq, sv, sh, conds = np.ones(B), np.ones(B), np.ones(B), np.ones(B)
    take = lambda x, at: None if x is None else np.asarray(x)[at]
    for d, at in _groups(desc, pi, _rows(B, rows)):
        H = OracleModel(d).crba(q[at])
        gq[at], gqd[at], gqdd[at], (sq[at], sv[at], sh[at]) = vc.rnea_vjp(d, q[at], take(qd, at), take(qdd, at), u[at], gravity, take(f_ext, at),
                                                                           consider_coriolis, consider_accelerations, H=H)
        conds[at] = [np.linalg.cond(h, np.inf) for h in H]
    gpi, sy, chi = pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, gravity, consider_coriolis, consider_accelerations, rows=rows)
    return gq, gqd, gqdd, gpi, (sq, sv, sh, sy, chi, conds)


def aba_parameters_state_vjp(desc, q, qd, tau, pi, w, gravity, f_ext=None, rows=None):
    """(qdd, gq, gqd, gtau [B, nv], gpi [B, n, 10], scales): scales = (|d qdd / d q|_inf, |d qdd / d qd|_inf, |H^-1|_inf, |H^-1 Y|_inf,
    chi, cond_inf(H(pi_r))), [B] each."""
    B, n, nv = q.shape[0], desc.n_joints, desc.nv
    pi = np.ascontiguousarray(pi, dtype=np.float64).reshape(B, n, 10)
    qdd, gq, gqd, gtau = np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv))
    sq, sv, sh = np.ones(B), np.ones(B), np.ones(B)
    take = lambda x, at: None if x is None else np.asarray(x)[at]
    for d, at in _groups(desc, pi, _rows(B, rows)):
        qdd[at], gq[at], gqd[at], gtau[at], (sq[at], sv[at], sh[at]) = vc.aba_vjp(d, q[at], qd[at], tau[at], w[at], gravity, take(f_ext, at))
    _, _, gpi, sy, chi, conds = pc.aba_parameters_vjp(desc, q, qd, tau, pi, w, gravity, f_ext, rows=rows)
    return qdd, gq, gqd, gtau, gpi, (sq, sv, sh, sy, chi, conds)
