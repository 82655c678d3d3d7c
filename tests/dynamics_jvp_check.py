"""CPU checker of the forward-mode calls (mh_rnea_jvp_*, mh_aba_jvp_*, mh_integrate_jvp_*, mh_aba_integrate_jvp_*): the matrices of
tests/dynamics_derivatives_check.py and tests/step_derivatives_check.py times the directions.  TEST INFRASTRUCTURE ONLY -- numpy, one
configuration at a time.

rnea_jvp / aba_jvp / integrate_jvp / step_jvp are the reference of every device result: nothing of the device's sweeps is used in them.
rnea_jvp_sweeps_one restates the device kernel's O(n) form (mh_rnea_jvp_kernels.h) in root coordinates with dense 6x6 matrices, where
motion_down and force_up are the identity; tests/test_dynamics_jvp_cpu.py holds it to the contraction, which is how the recursion is
checked without a GPU.
"""
from __future__ import annotations

import numpy as np

import dynamics_derivatives_check as dc
import step_derivatives_check as sc
from gravity_gradient_check import FIXED
from oracle import featherstone_np as fnp
from oracle.cpu_oracle import OracleModel


def _model(desc):
    return desc if isinstance(desc, dc.DerivativeModel) else dc.DerivativeModel(desc)


def _inf(M):
    return np.abs(M).max(axis=(1, 2))


def owned(m):
    own = np.zeros(m.nv, dtype=bool)
    for i in range(m.n):
        own[m.dofs(i)] = True
    return own


def _direction(m, B, d):
    """[B, nv] with zeros for a direction not given and at DoF indices no joint owns (the device does not read those)."""
    return np.zeros((B, m.nv)) if d is None else np.where(owned(m), np.asarray(d, dtype=float), 0.0)


def rnea_jvp(desc, q, qd, qdd, dq, dqd, dqdd, gravity, f_ext=None, consider_coriolis=True, consider_accelerations=True, rows=None, H=None):
    """(dtau [B, nv], scales): (d tau / d q) dq + (d tau / d qd) dqd + H dqdd; scales = the largest entries of the three matrices per
    configuration, [B] each.  Any direction may be None (zero).  desc: a ModelDesc (H from the oracle's crba unless given).  rows: the
    configurations to evaluate, the others stay zero."""
    m = _model(desc)
    q = np.asarray(q, dtype=float)
    B = q.shape[0]
    rows = list(range(B)) if rows is None else [int(r) for r in rows]
    qd_ = np.zeros((B, m.nv)) if qd is None else qd
    _, Dq, Dv = dc.rnea_derivatives(m, q, qd_, qdd, gravity, f_ext, consider_coriolis, consider_accelerations, rows=rows)
    if H is None:
        H = np.zeros((B, m.nv, m.nv))
        H[rows] = OracleModel(desc).crba(q[rows])
    keep = np.zeros((B, 1))
    keep[rows] = 1.0
    dtau = sum(np.einsum("bij,bj->bi", M, _direction(m, B, d)) for M, d in ((Dq, dq), (Dv, dqd), (H, dqdd))) * keep
    return dtau, (_inf(Dq), _inf(Dv), _inf(H))


def aba_jvp(desc, q, qd, tau, dq, dqd, dtau, gravity, f_ext=None, rows=None):
    """(qdd, dqdd [B, nv], scales): (d qdd / d q) dq + (d qdd / d qd) dqd + H^-1 dtau with the checker's forward-dynamics matrices;
    scales = the largest entries of those three matrices per configuration."""
    m = _model(desc)
    q = np.asarray(q, dtype=float)
    B = q.shape[0]
    qdd, Dq, Dv, Hinv = dc.aba_derivatives(m, q, qd, tau, gravity, f_ext, rows=rows)
    dqdd = sum(np.einsum("bij,bj->bi", M, _direction(m, B, d)) for M, d in ((Dq, dq), (Dv, dqd), (Hinv, dtau)))
    return qdd, dqdd, (_inf(Dq), _inf(Dv), _inf(Hinv))


def integrate_jvp_one(m, dt, qd, qdd, dq, dqd, dqdd):
    """(dq', dqd', abs-sums of the two) of one state: G_q dq + G_v dqd + G_a dqdd per joint, and the same on absolute terms."""
    out = [np.zeros(m.nv) for _ in range(4)]
    for i in range(m.n):
        t, di = int(m.type[i]), m.dofs(i)
        if t == FIXED:
            continue
        k = len(di)
        G, Gabs = sc.joint_blocks(t, dt, np.asarray(qd)[di], np.asarray(qdd)[di])
        x = sum(Gk @ d[di] for Gk, d in zip(G, (dq, dqd, dqdd)))
        xa = sum(Gk @ np.abs(d[di]) for Gk, d in zip(Gabs, (dq, dqd, dqdd)))
        out[0][di], out[1][di], out[2][di], out[3][di] = x[:k], x[k:], xa[:k], xa[k:]
    return tuple(out)


def integrate_jvp(desc, dt, qd, qdd, dq, dqd, dqdd):
    """(dq_next, dqd_next [B, nv], (abs-sums of the two)); any direction may be None (zero)."""
    m = _model(desc)
    qd = np.asarray(qd, dtype=float)
    B = qd.shape[0]
    a, b, c = (_direction(m, B, d) for d in (dq, dqd, dqdd))
    res = [integrate_jvp_one(m, dt, qd[r], np.asarray(qdd, dtype=float)[r], a[r], b[r], c[r]) for r in range(B)]
    cols = [np.stack([r[k] for r in res]) for k in range(4)]
    return cols[0], cols[1], tuple(cols[2:])


def step_jvp(desc, dt, q, qd, tau, dq, dqd, dtau, gravity, f_ext=None, rows=None):
    """(qdd, dqdd, dq_next, dqd_next [B, nv], (abs-sums of dq_next, dqd_next), (|A|_inf, |B|_inf [B]), scales of aba_jvp):
    (dq_next, dqd_next) = A (dq, dqd) + B dtau with the checker's (A, B) of the step; the abs-sums are A_abs |dx| + B_abs |dtau|.  rows: the
    configurations to evaluate, the others stay zero."""
    m = _model(desc)
    q = np.asarray(q, dtype=float)
    B, nv = q.shape[0], m.nv
    a, b, c = (_direction(m, B, d) for d in (dq, dqd, dtau))
    qdd, dqdd, dqn, dqdn, aq, av = (np.zeros((B, nv)) for _ in range(6))
    Ainf, Binf, sq, sv, sh = (np.zeros(B) for _ in range(5))
    for r in (range(B) if rows is None else rows):
        fe = None if f_ext is None else np.asarray(f_ext)[r]
        qdd[r], Dq, Dv, Hinv = dc.aba_derivatives_one(m, q[r], np.asarray(qd)[r], np.asarray(tau)[r], gravity, fe)
        A, Bm, Aa, Ba = sc.assemble_one(m, dt, np.asarray(qd)[r], qdd[r], Dq, Dv, Hinv)
        dx = np.concatenate([a[r], b[r]])
        x, xa = A @ dx + Bm @ c[r], Aa @ np.abs(dx) + Ba @ np.abs(c[r])
        dqdd[r] = Dq @ a[r] + Dv @ b[r] + Hinv @ c[r]
        dqn[r], dqdn[r], aq[r], av[r] = x[:nv], x[nv:], xa[:nv], xa[nv:]
        Ainf[r], Binf[r] = np.abs(A).max(), np.abs(Bm).max()
        sq[r], sv[r], sh[r] = np.abs(Dq).max(), np.abs(Dv).max(), np.abs(Hinv).max()
    return qdd, dqdd, dqn, dqdn, (aq, av), (Ainf, Binf), (sq, sv, sh)


def rnea_jvp_sweeps_one(m: dc.DerivativeModel, q, qd, qdd, dq, dqd, dqdd, gravity, f_ext=None, tau_in=None):
    """dtau of one state by the kernel's two sweeps.  Every tangent is the BODY-FIXED derivative of the kernel (the frame of body j moves
    with its displacement twist xi_j), written in root coordinates, where motion_down and force_up are the identity:
        outward  xi_j = xi_p + S dq_j
                 dv_j = dv_p + v_p x S dq_j + S dqd_j
                 da_j = da_p + a_p x S dq_j + S dqdd_j + dv_j x vJ_j + v_j x S dqd_j          (a_p = the root acceleration above the root)
                 df_j = I da + dv x* (I v) + v x* (I dv) + xi x* fe
        inward   dF_j = df_j + sum_children (dF_c + (S dq_c) x* F_c),   dtau_j = S_j^T dF_j
    tau_in: the result is tau_in - dtau (the right-hand side of the forward form)."""
    qd, qdd = np.asarray(qd, dtype=float), np.asarray(qdd, dtype=float)
    a0, S, v, a, I, _, f, fe = dc._state(m, q, qd, qdd, gravity, f_ext)
    n, z = m.n, np.zeros(6)
    Sq = [S[j] @ np.asarray(dq, dtype=float)[m.dofs(j)] for j in range(n)]
    Sv = [S[j] @ np.asarray(dqd, dtype=float)[m.dofs(j)] for j in range(n)]
    Sa = [S[j] @ np.asarray(dqdd, dtype=float)[m.dofs(j)] for j in range(n)]
    xi, dv, da, dF = [None] * n, [None] * n, [None] * n, [None] * n
    for j in range(n):  # outward
        p = m.parent[j]
        vp, ap, xip, dvp, dap = (z, a0, z, z, z) if p < 0 else (v[p], a[p], xi[p], dv[p], da[p])
        vJ = S[j] @ qd[m.dofs(j)]
        xi[j] = xip + Sq[j]
        dv[j] = dvp + fnp.crm(vp) @ Sq[j] + Sv[j]
        da[j] = dap + fnp.crm(ap) @ Sq[j] + Sa[j] + fnp.crm(dv[j]) @ vJ + fnp.crm(v[j]) @ Sv[j]
        dF[j] = I[j] @ da[j] + fnp.crf(dv[j]) @ (I[j] @ v[j]) + fnp.crf(v[j]) @ (I[j] @ dv[j]) + fnp.crf(xi[j]) @ fe[j]
    F = [x.copy() for x in f]
    dtau = np.zeros(m.nv)
    for j in range(n - 1, -1, -1):  # inward: the children of j have handed theirs over
        dtau[m.dofs(j)] = S[j].T @ dF[j]
        p = m.parent[j]
        if p >= 0:
            dF[p] = dF[p] + dF[j] + fnp.crf(Sq[j]) @ F[j]
            F[p] = F[p] + F[j]
    if tau_in is not None:
        return np.where(owned(m), np.asarray(tau_in, dtype=float) - dtau, 0.0)
    return dtau
