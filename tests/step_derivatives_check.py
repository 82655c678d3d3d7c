"""CPU checker of mh_configuration_add_*, mh_configuration_difference_* and mh_aba_integrate_derivatives_*: numpy, one configuration at a
time, every joint kind.  TEST INFRASTRUCTURE ONLY.

(+) is MultiBodySystemStateIntegrator.integrateFromVelocity with dt = 1 (tools/MultiBodySystemStateIntegrator.java:164-243), (-) its
inverse.  The linearisation of the step "forward dynamics, then the constant-acceleration integrator" is assembled from
dynamics_derivatives_check.aba_derivatives_one and, per joint, three dense blocks G_q, G_v, G_a [2k, k] (rows: the joint's dq', then its
dqd'; columns: its dq, dqd, dqdd), written out as block matrices of E^T = exp(r)^T, J_r(r) and skew matrices -- not as the chain of
vector operations the device applies.  Beside every matrix the sum of the absolute values of the terms that went into each entry is
carried along (the same formulas on absolute values with every sign a plus): the rounding bound of the device test is a multiple of it.
tests/test_step_derivatives_cpu.py pins this file against the C oracle's step and central differences of it.
"""
from __future__ import annotations

import math

import numpy as np

import dynamics_derivatives_check as dc
from gravity_gradient_check import FIXED, PLANAR, PRISMATIC, REVOLUTE, SIXDOF, SPHERICAL
from oracle import featherstone_np as fnp

StepModel = dc.DerivativeModel


def _model(desc):
    return desc if isinstance(desc, dc.DerivativeModel) else dc.DerivativeModel(desc)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _series(th2, first):
    """sum_k (-1)^k th^(2k) / (2k + first)!"""
    return sum((-1.0) ** k * th2 ** k / math.factorial(2 * k + first) for k in range(14))


def so3_coefficients(th):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3): Taylor sums below 1/2, closed forms above."""
    if th < 0.5:
        return _series(th * th, 1), _series(th * th, 2), _series(th * th, 3)
    return math.sin(th) / th, (1.0 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3


def exp_and_right_jacobian(r):
    """(E, J_r, |E| terms, |J_r| terms) of the rotation vector r; E is the identity below the step's own threshold |r| = 1e-12."""
    th = float(np.linalg.norm(r))
    K, Ka = skew(r), np.abs(skew(r))
    a, b, c = so3_coefficients(th)
    if th < 1.0e-12:
        return np.eye(3), np.eye(3) - b * K, np.eye(3), np.eye(3) + b * Ka
    return np.eye(3) + a * K + b * K @ K, np.eye(3) - b * K + c * K @ K, np.eye(3) + a * Ka + b * Ka @ Ka, np.eye(3) + b * Ka + c * Ka @ Ka


def quat_mul(a, b):
    """Hamilton product of (x, y, z, s) quaternions."""
    ax, ay, az, as_ = a
    bx, by, bz, bs = b
    return np.array([as_ * bx + ax * bs + ay * bz - az * by, as_ * by - ax * bz + ay * bs + az * bx, as_ * bz + ax * by - ay * bx + az * bs,
                     as_ * bs - ax * bx - ay * by - az * bz])


def quat_exp(r):
    th = float(np.linalg.norm(r))
    if th < 1.0e-12:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(0.5 * th) / th * np.asarray(r), [np.cos(0.5 * th)]])


def quat_log(Q):
    """Rotation vector of a unit quaternion, |.| <= pi."""
    Q = np.asarray(Q, dtype=float)
    if Q[3] < 0.0:
        Q = -Q
    n = float(np.linalg.norm(Q[:3]))
    return 2.0 * Q[:3] / Q[3] if n == 0.0 else 2.0 * math.atan2(n, Q[3]) / n * Q[:3]


def _cfg(m, i):
    return m.cfg_idx[m.cfg_ofs[i]:m.cfg_ofs[i + 1]]


def configuration_add_one(m, q, dq):
    q = np.asarray(q, dtype=float)
    out = q.copy()
    for i in range(m.n):
        t, ci, di = int(m.type[i]), _cfg(m, i), m.dofs(i)
        if t in (REVOLUTE, PRISMATIC):
            out[ci[0]] = q[ci[0]] + dq[di[0]]
        elif t == PLANAR:
            c, s = math.cos(q[ci[0]]), math.sin(q[ci[0]])
            out[ci[0]] = q[ci[0]] + dq[di[0]]
            out[ci[1]] = q[ci[1]] + c * dq[di[1]] + s * dq[di[2]]
            out[ci[2]] = q[ci[2]] - s * dq[di[1]] + c * dq[di[2]]
        elif t in (SPHERICAL, SIXDOF):
            out[ci[:4]] = quat_mul(q[ci[:4]], quat_exp(dq[di[:3]]))
            if t == SIXDOF:
                out[ci[4:7]] = q[ci[4:7]] + fnp.quat_to_R(q[ci[:4]]) @ dq[di[3:6]]
    return out


def configuration_difference_one(m, q0, q1):
    q0, q1 = np.asarray(q0, dtype=float), np.asarray(q1, dtype=float)
    out = np.zeros(m.nv)
    for i in range(m.n):
        t, ci, di = int(m.type[i]), _cfg(m, i), m.dofs(i)
        if t in (REVOLUTE, PRISMATIC):
            out[di[0]] = q1[ci[0]] - q0[ci[0]]
        elif t == PLANAR:
            c, s = math.cos(q0[ci[0]]), math.sin(q0[ci[0]])
            dx, dz = q1[ci[1]] - q0[ci[1]], q1[ci[2]] - q0[ci[2]]
            out[di[0]], out[di[1]], out[di[2]] = q1[ci[0]] - q0[ci[0]], c * dx - s * dz, s * dx + c * dz
        elif t in (SPHERICAL, SIXDOF):
            a, b = q0[ci[:4]] / np.linalg.norm(q0[ci[:4]]), q1[ci[:4]] / np.linalg.norm(q1[ci[:4]])
            out[di[:3]] = quat_log(quat_mul(np.concatenate([-a[:3], a[3:]]), b))
            if t == SIXDOF:
                out[di[3:6]] = fnp.quat_to_R(a).T @ (q1[ci[4:7]] - q0[ci[4:7]])
    return out


def configuration_add(desc, q, dq):
    m = _model(desc)
    return np.stack([configuration_add_one(m, a, b) for a, b in zip(np.asarray(q, dtype=float), np.asarray(dq, dtype=float))])


def configuration_difference(desc, q0, q1):
    m = _model(desc)
    return np.stack([configuration_difference_one(m, a, b) for a, b in zip(np.asarray(q0, dtype=float), np.asarray(q1, dtype=float))])


_EMBED = {SIXDOF: [0, 1, 2, 3, 4, 5], SPHERICAL: [0, 1, 2], PLANAR: [1, 3, 5]}  # the joint's DoFs among (w, v) of a 6-DoF joint


def joint_blocks(t, dt, vj, aj):
    """(G_q, G_v, G_a) of one joint, each [2k, k], and the same three with absolute terms; vj, aj: the joint's entries of qd and qdd."""
    h = 0.5 * dt * dt
    if t in (REVOLUTE, PRISMATIC):
        G = (np.array([[1.0], [0.0]]), np.array([[dt], [1.0]]), np.array([[h], [dt]]))
        return G, tuple(np.abs(g) for g in G)
    sel = _EMBED[t]
    tw, ac = np.zeros(6), np.zeros(6)
    tw[sel], ac[sel] = vj, aj
    w, v, al, a = tw[:3], tw[3:], ac[:3], ac[3:]
    a_o = a + np.cross(w, v)
    a_o_abs = np.abs(a) + np.abs(skew(w)) @ np.abs(v)
    E, Jr, Ea, Ja = exp_and_right_jacobian(dt * w + h * al)
    Et, Eta = E.T, Ea.T
    d = dt * v + h * a_o
    d_abs = abs(dt) * np.abs(v) + h * a_o_abs
    vn = Et @ (v + dt * a_o)
    vn_abs = Eta @ (np.abs(v) + abs(dt) * a_o_abs)
    I3, Z = np.eye(3), np.zeros((3, 3))
    S = lambda x: skew(x)
    Sa = lambda x: np.abs(skew(x))
    adt = abs(dt)
    Gq = np.block([[Et, Z], [-Et @ S(d), Et], [Z, Z], [Z, Z]])
    Gq_abs = np.block([[Eta, Z], [Eta @ Sa(d_abs), Eta], [Z, Z], [Z, Z]])
    Gv = np.block([[dt * Jr, Z], [-h * Et @ S(v), Et @ (dt * I3 + h * S(w))],
                   [I3, Z], [dt * S(vn) @ Jr - dt * Et @ S(v), Et @ (I3 + dt * S(w))]])
    Gv_abs = np.block([[adt * Ja, Z], [h * Eta @ Sa(v), Eta @ (adt * I3 + h * Sa(w))],
                       [I3, Z], [adt * Sa(vn_abs) @ Ja + adt * Eta @ Sa(v), Eta @ (I3 + adt * Sa(w))]])
    Ga = np.block([[h * Jr, Z], [Z, h * Et], [dt * I3, Z], [h * S(vn) @ Jr, dt * Et]])
    Ga_abs = np.block([[h * Ja, Z], [Z, h * Eta], [adt * I3, Z], [h * Sa(vn_abs) @ Ja, adt * Eta]])
    rows = sel + [6 + s for s in sel]
    pick = lambda G: G[np.ix_(rows, sel)]
    return (pick(Gq), pick(Gv), pick(Ga)), (pick(Gq_abs), pick(Gv_abs), pick(Ga_abs))


def assemble_one(m, dt, qd, qdd, Dq, Dv, Hinv):
    """(A [2nv, 2nv], B [2nv, nv], A_abs, B_abs) from the state's (qd, qdd) and the three matrices of the forward-dynamics derivatives."""
    nv = m.nv
    A, Bm, Aa, Ba = np.zeros((2 * nv, 2 * nv)), np.zeros((2 * nv, nv)), np.zeros((2 * nv, 2 * nv)), np.zeros((2 * nv, nv))
    D, Da, Ha = np.hstack([Dq, Dv]), np.abs(np.hstack([Dq, Dv])), np.abs(Hinv)
    for i in range(m.n):
        t, di = int(m.type[i]), m.dofs(i)
        if t == FIXED:
            continue
        k = len(di)
        (Gq, Gv, Ga), (Gqa, Gva, Gaa) = joint_blocks(t, dt, np.asarray(qd)[di], np.asarray(qdd)[di])
        rows = np.concatenate([di, nv + di])
        A[rows] += Ga @ D[di]
        Aa[rows] += Gaa @ Da[di]
        A[np.ix_(rows, di)] += Gq
        Aa[np.ix_(rows, di)] += Gqa
        A[np.ix_(rows, nv + di)] += Gv
        Aa[np.ix_(rows, nv + di)] += Gva
        Bm[rows] = Ga @ Hinv[di]
        Ba[rows] = Gaa @ Ha[di]
    return A, Bm, Aa, Ba


def step_derivatives_one(m, dt, q, qd, tau, gravity, f_ext=None, H=None):
    """(qdd, A, B, A_abs, B_abs) of one state."""
    qdd, Dq, Dv, Hinv = dc.aba_derivatives_one(m, q, qd, tau, gravity, f_ext, H=H)
    return (qdd,) + assemble_one(m, dt, qd, qdd, Dq, Dv, Hinv)


def step_derivatives(desc, dt, q, qd, tau, gravity, f_ext=None, rows=None):
    """Batched front end: (qdd [B, nv], A [B, 2nv, 2nv], B [B, 2nv, nv]); rows: the configurations to evaluate (the others stay zero)."""
    m = _model(desc)
    q = np.asarray(q, dtype=float)
    n, nv = q.shape[0], m.nv
    qdd, A, Bm = np.zeros((n, nv)), np.zeros((n, 2 * nv, 2 * nv)), np.zeros((n, 2 * nv, nv))
    for b in (range(n) if rows is None else rows):
        qdd[b], A[b], Bm[b], _, _ = step_derivatives_one(m, dt, q[b], np.asarray(qd)[b], np.asarray(tau)[b], gravity,
                                                         None if f_ext is None else np.asarray(f_ext)[b])
    return qdd, A, Bm
