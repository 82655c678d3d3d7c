"""CPU checker of the dynamics-derivative calls (mh_rnea_derivatives_*, mh_aba_derivatives_*): an analytic numpy restatement, one
configuration at a time, for every joint kind.  TEST INFRASTRUCTURE ONLY.

Everything is written in ONE frame, the root body's, with dense 6x6 matrices -- not in the joint frames and not with the composite
quantities the device kernel collapses the sums into.  The poses are gravity_gradient_check.GravityModel's.  With s the unit twist of a
DoF of joint j (root coordinates), a velocity-space step along it moves the subtree of j rigidly by s while the COMPONENTS of qd and qdd
stay what they were, and the external wrenches stay where they are in the world.  For every body k of that subtree

    dv_k = s x v_k + psid,                         psid  = v_parent(j) x s
    da_k = s x a_k + psidd + psid x v_k,           psidd = a_parent(j) x s + v_parent(j) x psid
    df_k = s x* (f_k + fext_k) + I_k psidd + B_k psid,   B_k = v_k x* I_k - I_k v_k x + (I_k v_k) xbar*   (f xbar* m := m x* f)

and a step of qd along the same DoF gives  da_k = s x v_k + psid + v_j x s,  df_k = B_k s + I_k (psid + v_j x s).  The effort of DoF r of
joint i is tau = S_r . sum of f_k over the subtree of i, and S_r moves with s too (dS_r = s x S_r) when i lies in the subtree of j.  The
sums over the bodies are taken as they stand: O(n^2) per column, nothing shared with the device's three sweeps.
tests/test_dynamics_derivatives_cpu.py pins this file against the C oracle's inverse and forward dynamics and their central differences,
and at rest against gravity_gradient_check.
"""
from __future__ import annotations

import numpy as np

from gravity_gradient_check import GravityModel
from oracle import featherstone_np as fnp


class DerivativeModel(GravityModel):
    def __init__(self, desc):
        super().__init__(desc)
        n = self.n
        J = np.asarray(desc.inertia_J, dtype=float).reshape(n, 3, 3)
        self.I = []  # 6x6 inertia of every body about the origin of the frame after its joint, in that frame
        for i in range(n):
            Rc, pc = self.Xc[i, :9].reshape(3, 3), self.Xc[i, 9:]
            c = self.com[i]
            J_com = J[i] - self.mass[i] * (fnp.skew(c) @ fnp.skew(c).T)  # desc.inertia_J is about the body-fixed origin
            self.I.append(fnp.spatial_inertia(Rc @ J_com @ Rc.T, self.mass[i], Rc @ c + pc))
        self.subtree = [[i] for i in range(n)]
        for i in range(n - 1, -1, -1):
            if self.parent[i] >= 0:
                self.subtree[self.parent[i]] += self.subtree[i]


def _bar(f):
    """6x6 matrix of m -> m x* f."""
    return np.stack([fnp.crf(e) @ f for e in np.eye(6)], axis=1)


def _state(m: DerivativeModel, q, qd, qdd, gravity, f_ext):
    """Per body, in root coordinates: S [6, nd], v, a, inertia, B, body force f, external force."""
    n = m.n
    Ra, pa, Rf, pf = m.world_poses(np.asarray(q, dtype=float))
    a0 = fnp._root_acceleration(gravity)
    S, v, a, I, Bm, f, fe = [], [], [], [], [], [], []
    for i in range(n):
        X0 = fnp.plucker_motion(Ra[i], pa[i])  # motion, frame after joint i -> root
        Xf = np.linalg.inv(X0).T               # force, the same way
        tw = m.unit_twists(i)
        S.append(X0 @ np.array([np.concatenate(t) for t in tw]).T if tw else np.zeros((6, 0)))
        p = m.parent[i]
        vJ = S[i] @ qd[m.dofs(i)]
        v.append((np.zeros(6) if p < 0 else v[p]) + vJ)
        a.append((a0 if p < 0 else a[p]) + S[i] @ qdd[m.dofs(i)] + fnp.crm(v[i]) @ vJ)
        I.append(Xf @ m.I[i] @ Xf.T)
        fe.append(np.zeros(6) if f_ext is None else np.linalg.inv(fnp.plucker_motion(Rf[i], pf[i])).T @ np.asarray(f_ext[i], dtype=float))
        hv = I[i] @ v[i]
        f.append(I[i] @ a[i] + fnp.crf(v[i]) @ hv - fe[i])
        Bm.append(fnp.crf(v[i]) @ I[i] - I[i] @ fnp.crm(v[i]) + _bar(hv))
    return a0, S, v, a, I, Bm, f, fe


def rnea_derivatives_one(m: DerivativeModel, q, qd, qdd, gravity, f_ext=None, consider_coriolis=True, consider_accelerations=True):
    """(tau [nv], dtau_dq [nv, nv], dtau_dqd [nv, nv]) of one state.  gravity: 3-vector, or the root's 6-D spatial acceleration."""
    qd = np.asarray(qd, dtype=float) if consider_coriolis else np.zeros(m.nv)
    qdd = np.asarray(qdd, dtype=float) if consider_accelerations else np.zeros(m.nv)
    a0, S, v, a, I, Bm, f, fe = _state(m, q, qd, qdd, gravity, f_ext)
    n, nv = m.n, m.nv
    Fc = [sum(f[k] for k in m.subtree[i]) for i in range(n)]
    tau, dq, dqd = np.zeros(nv), np.zeros((nv, nv)), np.zeros((nv, nv))
    for i in range(n):
        tau[m.dofs(i)] = S[i].T @ Fc[i]
    for j in range(n):
        p = m.parent[j]
        vp, ap = (np.zeros(6), a0) if p < 0 else (v[p], a[p])
        inside = set(m.subtree[j])
        for c, col in enumerate(m.dofs(j)):
            s = S[j][:, c]
            psid = fnp.crm(vp) @ s
            psidd = fnp.crm(ap) @ s + fnp.crm(vp) @ psid
            sd = fnp.crm(v[j]) @ s
            df_q = {k: fnp.crf(s) @ (f[k] + fe[k]) + I[k] @ psidd + Bm[k] @ psid for k in inside}
            df_v = {k: Bm[k] @ s + I[k] @ (psid + sd) for k in inside}
            z = np.zeros(6)
            for i in range(n):
                common = [k for k in m.subtree[i] if k in inside]
                if not common:
                    continue  # neither is an ancestor of the other: the entries stay exactly zero
                di = m.dofs(i)
                dq[di, col] = S[i].T @ sum((df_q[k] for k in common), z)
                dqd[di, col] = S[i].T @ sum((df_v[k] for k in common), z)
                if i in inside:
                    dq[di, col] += (fnp.crm(s) @ S[i]).T @ Fc[i]
    return tau, dq, dqd


def mass_matrix_one(m: DerivativeModel, q):
    _, S, _, _, I, _, _, _ = _state(m, q, np.zeros(m.nv), np.zeros(m.nv), np.zeros(3), None)
    H = np.zeros((m.nv, m.nv))
    for i in range(m.n):
        for j in range(m.n):
            common = [k for k in m.subtree[i] if k in set(m.subtree[j])]
            if common:
                H[np.ix_(m.dofs(i), m.dofs(j))] = S[i].T @ sum(I[k] for k in common) @ S[j]
    return H


def aba_derivatives_one(m: DerivativeModel, q, qd, tau, gravity, f_ext=None, H=None, qdd=None):
    """(qdd, dqdd_dq, dqdd_dqd, Hinv) of one state: qdd from H qdd = tau - rnea(q, qd, 0) unless given, the derivatives -Hinv dtau/d(.)
    of the inverse dynamics at that qdd."""
    if H is None:
        H = mass_matrix_one(m, q)
    Hinv = np.linalg.inv(H)
    if qdd is None:
        bias, _, _ = rnea_derivatives_one(m, q, qd, np.zeros(m.nv), gravity, f_ext)
        qdd = Hinv @ (np.asarray(tau, dtype=float) - bias)
    _, dq, dqd = rnea_derivatives_one(m, q, qd, qdd, gravity, f_ext)
    return qdd, -Hinv @ dq, -Hinv @ dqd, Hinv


def _model(desc):
    return desc if isinstance(desc, DerivativeModel) else DerivativeModel(desc)


def rnea_derivatives(desc, q, qd, qdd, gravity, f_ext=None, consider_coriolis=True, consider_accelerations=True, rows=None):
    """Batched front end: (tau [B, nv], dtau_dq [B, nv, nv], dtau_dqd [B, nv, nv]).  rows: the configurations to evaluate (the others
    stay zero), for models on which one evaluation takes seconds."""
    m = _model(desc)
    q = np.asarray(q, dtype=float)
    B = q.shape[0]
    tau, dq, dqd = np.zeros((B, m.nv)), np.zeros((B, m.nv, m.nv)), np.zeros((B, m.nv, m.nv))
    for b in (range(B) if rows is None else rows):
        tau[b], dq[b], dqd[b] = rnea_derivatives_one(m, q[b], np.asarray(qd)[b], None if qdd is None else np.asarray(qdd)[b], gravity,
                                                     None if f_ext is None else np.asarray(f_ext)[b], consider_coriolis,
                                                     consider_accelerations and qdd is not None)
    return tau, dq, dqd


def aba_derivatives(desc, q, qd, tau, gravity, f_ext=None, rows=None):
    """Batched front end: (qdd [B, nv], dqdd_dq, dqdd_dqd, Hinv [B, nv, nv])."""
    m = _model(desc)
    q = np.asarray(q, dtype=float)
    B = q.shape[0]
    qdd, dq, dqd, Hinv = np.zeros((B, m.nv)), np.zeros((B, m.nv, m.nv)), np.zeros((B, m.nv, m.nv)), np.zeros((B, m.nv, m.nv))
    for b in (range(B) if rows is None else rows):
        qdd[b], dq[b], dqd[b], Hinv[b] = aba_derivatives_one(m, q[b], np.asarray(qd)[b], np.asarray(tau)[b], gravity,
                                                             None if f_ext is None else np.asarray(f_ext)[b])
    return qdd, dq, dqd, Hinv
