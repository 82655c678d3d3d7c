"""CPU checker of the reverse-mode gradient calls (mh_rnea_vjp_*, mh_aba_vjp_*): the matrices of tests/dynamics_derivatives_check.py
contracted with the cotangent, and H u with H from the C oracle's crba.  TEST INFRASTRUCTURE ONLY -- numpy, one configuration at a time.

rnea_vjp / aba_vjp are the reference of every device result: nothing of the device's sweeps is used in them.  rnea_vjp_sweeps_one restates
the device kernel's O(n) form (mh_rnea_vjp_kernels.h) in root coordinates with dense 6x6 matrices, where motion_down and force_up are
the identity; tests/test_dynamics_vjp_cpu.py holds it to the contraction, which is how the identities are checked without a GPU.
"""
from __future__ import annotations

import numpy as np

import dynamics_derivatives_check as dc
from oracle import featherstone_np as fnp
from oracle.cpu_oracle import OracleModel


def _model(desc):
    return desc if isinstance(desc, dc.DerivativeModel) else dc.DerivativeModel(desc)


def _inf(M):
    return np.abs(M).max(axis=(1, 2))


def rnea_vjp(desc, q, qd, qdd, u, gravity, f_ext=None, consider_coriolis=True, consider_accelerations=True, rows=None, H=None):
    """(gq, gqd, gqdd [B, nv], scales): u^T d tau / d q, u^T d tau / d qd and H u; scales = the largest entries of d tau / d q, d tau / d qd
    and H per configuration, [B] each (what the bounds of the GPU tests scale with).  desc: a ModelDesc (H from the oracle's crba unless
    given).  rows: the configurations to evaluate, the others stay zero."""
    m = _model(desc)
    q, u = np.asarray(q, dtype=float), np.asarray(u, dtype=float)
    B = q.shape[0]
    rows = list(range(B)) if rows is None else [int(r) for r in rows]
    _, dq, dqd = dc.rnea_derivatives(m, q, qd, qdd, gravity, f_ext, consider_coriolis, consider_accelerations, rows=rows)
    if H is None:
        H = np.zeros((B, m.nv, m.nv))
        H[rows] = OracleModel(desc).crba(q[rows])
    keep = np.zeros((B, 1))
    keep[rows] = 1.0
    gq, gqd, gqdd = (np.einsum("bi,bij->bj", u, M) * keep for M in (dq, dqd, H))
    return gq, gqd, gqdd, (_inf(dq), _inf(dqd), _inf(H))


def aba_vjp(desc, q, qd, tau, w, gravity, f_ext=None, rows=None):
    """(qdd, gq, gqd, gtau [B, nv], scales): w^T d qdd / d q, w^T d qdd / d qd and w^T H^-1 with the checker's forward-dynamics matrices;
    scales = the largest entries of those three matrices per configuration."""
    m = _model(desc)
    q, w = np.asarray(q, dtype=float), np.asarray(w, dtype=float)
    qdd, dq, dqd, Hinv = dc.aba_derivatives(m, q, qd, tau, gravity, f_ext, rows=rows)
    gq, gqd, gtau = (np.einsum("bi,bij->bj", w, M) for M in (dq, dqd, Hinv))
    return qdd, gq, gqd, gtau, (_inf(dq), _inf(dqd), _inf(Hinv))


def rnea_vjp_sweeps_one(m: dc.DerivativeModel, q, qd, qdd, u, gravity, f_ext=None):
    """(gq, gqd, gqdd) of one state by the kernel's two sweeps, in root coordinates:
        nu_j = nu_parent + S_j u_j,   nul_j = nu_parent
        T1b_j, T4b_j, T5b_j = sums over the strict descendants d of Ic_d (S_d u_d), BSc_d^T (S_d u_d), -(S_d u_d) x* Wc_d
        X1 = T1b + Ic nu,  X4 = T4b + BSc^T nu,  X5 = T5b - nu x* Wc - nul x* Fc
        gq = S^T (X5 - vl x* (X4 - vl x* X1) - al x* X1),  gqd = S^T (X4 - (vl + v) x* X1),  gqdd = S^T X1."""
    a0, S, v, a, I, Bm, f, fe = dc._state(m, q, np.asarray(qd, dtype=float), np.asarray(qdd, dtype=float), gravity, f_ext)
    n, z = m.n, np.zeros(6)
    u = np.asarray(u, dtype=float)
    Su = [S[j] @ u[m.dofs(j)] for j in range(n)]
    nu = [None] * n
    for j in range(n):  # outward
        nu[j] = (z if m.parent[j] < 0 else nu[m.parent[j]]) + Su[j]
    Ic, Bc, Fc, Wc = [x.copy() for x in I], [x.copy() for x in Bm], [x.copy() for x in f], [x.copy() for x in fe]
    T1, T4, T5 = [z.copy() for _ in range(n)], [z.copy() for _ in range(n)], [z.copy() for _ in range(n)]
    gq, gqd, gqdd = np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nv)
    for j in range(n - 1, -1, -1):  # inward: the children of j have handed theirs over
        p = m.parent[j]
        vl, al, nul = (z, a0, z) if p < 0 else (v[p], a[p], nu[p])
        X1 = T1[j] + Ic[j] @ nu[j]
        X4 = T4[j] + Bc[j].T @ nu[j]
        X5 = T5[j] - fnp.crf(nu[j]) @ Wc[j] - fnp.crf(nul) @ Fc[j]
        d = m.dofs(j)
        gq[d] = S[j].T @ (X5 - fnp.crf(vl) @ (X4 - fnp.crf(vl) @ X1) - fnp.crf(al) @ X1)
        gqd[d] = S[j].T @ (X4 - fnp.crf(vl + v[j]) @ X1)
        gqdd[d] = S[j].T @ X1
        if p >= 0:
            T1[p] += T1[j] + Ic[j] @ Su[j]
            T4[p] += T4[j] + Bc[j].T @ Su[j]
            T5[p] += T5[j] - fnp.crf(Su[j]) @ Wc[j]
            Ic[p] += Ic[j]
            Bc[p] += Bc[j]
            Fc[p] += Fc[j]
            Wc[p] += Wc[j]
    return gq, gqd, gqdd
