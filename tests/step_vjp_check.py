"""CPU checker of mh_integrate_vjp_* and mh_aba_integrate_vjp_*: the transposes of the matrices of tests/step_derivatives_check.py
applied to the cotangents.  TEST INFRASTRUCTURE ONLY -- numpy, one configuration at a time.

integrate_vjp / step_vjp are the reference of every device result: nothing of the device's vector form is used in them.  Beside every
value the same contraction of the absolute terms with |g'| is carried along (the rounding bound of the device test is a multiple of
it).  joint_vjp_vector_form restates the kernel's chain of vector operations (mh_step_kernels.h: step_apply_t); tests/test_step_vjp_cpu.py
holds it to the transposed blocks, which is how the identities are checked without a GPU.
"""
from __future__ import annotations

import numpy as np

import step_derivatives_check as sc
from gravity_gradient_check import FIXED, PRISMATIC, REVOLUTE


def _owned(m):
    own = np.zeros(m.nv, dtype=bool)
    for i in range(m.n):
        own[m.dofs(i)] = True
    return own


def _cotangent(m, B, g, own):
    """[B, nv] with zeros for a cotangent not given and at DoF indices no joint owns (the device does not read those)."""
    return np.zeros((B, m.nv)) if g is None else np.where(own, np.asarray(g, dtype=float), 0.0)


def integrate_vjp_one(m, dt, qd, qdd, ga, gb):
    """(gq, gqd, gqdd, gq_abs, gqd_abs, gqdd_abs) of one state: G^T g' per joint, and |G|_abs^T |g'|."""
    out = [np.zeros(m.nv) for _ in range(6)]
    for i in range(m.n):
        t, di = int(m.type[i]), m.dofs(i)
        if t == FIXED:
            continue
        G, Gabs = sc.joint_blocks(t, dt, np.asarray(qd)[di], np.asarray(qdd)[di])
        g = np.concatenate([ga[di], gb[di]])
        for k in range(3):
            out[k][di] = G[k].T @ g
            out[3 + k][di] = Gabs[k].T @ np.abs(g)
    return tuple(out)


def integrate_vjp(desc, dt, qd, qdd, gq_next, gqd_next):
    """(gq, gqd, gqdd [B, nv], (abs-sums of the three)); either cotangent may be None (zero)."""
    m = sc._model(desc)
    qd = np.asarray(qd, dtype=float)
    B, own = qd.shape[0], _owned(m)
    ga, gb = _cotangent(m, B, gq_next, own), _cotangent(m, B, gqd_next, own)
    res = [integrate_vjp_one(m, dt, qd[b], np.asarray(qdd, dtype=float)[b], ga[b], gb[b]) for b in range(B)]
    cols = [np.stack([r[k] for r in res]) for k in range(6)]
    return cols[0], cols[1], cols[2], tuple(cols[3:])


def step_vjp(desc, dt, q, qd, tau, gq_next, gqd_next, gravity, f_ext=None, rows=None):
    """(qdd, gq, gqd, gtau [B, nv], (abs-sums of gq, gqd, gtau), (|A|_inf, |B|_inf [B])): (gq, gqd) = A^T g', gtau = B^T g' with the
    checker's (A, B) of the step; the abs-sums are A_abs^T |g'| and B_abs^T |g'|.  rows: the configurations to evaluate, the others stay
    zero."""
    m = sc._model(desc)
    q = np.asarray(q, dtype=float)
    B, nv, own = q.shape[0], m.nv, _owned(m)
    ga, gb = _cotangent(m, B, gq_next, own), _cotangent(m, B, gqd_next, own)
    qdd, gq, gqd, gtau, aq, av, at = (np.zeros((B, nv)) for _ in range(7))
    Ainf, Binf = np.zeros(B), np.zeros(B)
    for b in (range(B) if rows is None else rows):
        qdd[b], A, Bm, Aa, Ba = sc.step_derivatives_one(m, dt, q[b], np.asarray(qd)[b], np.asarray(tau)[b], gravity,
                                                        None if f_ext is None else np.asarray(f_ext)[b])
        g = np.concatenate([ga[b], gb[b]])
        x, xa = A.T @ g, Aa.T @ np.abs(g)
        gq[b], gqd[b], gtau[b] = x[:nv], x[nv:], Bm.T @ g
        aq[b], av[b], at[b] = xa[:nv], xa[nv:], Ba.T @ np.abs(g)
        Ainf[b], Binf[b] = np.abs(A).max(), np.abs(Bm).max()
    return qdd, gq, gqd, gtau, (aq, av, at), (Ainf, Binf)


def joint_vjp_vector_form(t, dt, vj, aj, ga, gb):
    """(gq, gqd, gqdd) of one joint [k each] by the kernel's chain of vector operations:
        P = E gp',  V = E gv',  s = J_r^T (gth' + gv' x vn),  g_ao = h P + dt V
        gq = (E gth' + d x P, P),  gqd = (gw' + dt s + v x g_ao, dt P + V + g_ao x w),  gqdd = (dt gw' + h s, g_ao)
    a spherical joint the rotational half, a planar joint the restriction to (w_y, v_x, v_z), a 1-DoF joint scalars."""
    h = 0.5 * dt * dt
    if t in (REVOLUTE, PRISMATIC):
        return np.array([ga[0]]), np.array([dt * ga[0] + gb[0]]), np.array([h * ga[0] + dt * gb[0]])
    sel = sc._EMBED[t]
    tw, ac, a6, b6 = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6)
    tw[sel], ac[sel], a6[sel], b6[sel] = vj, aj, ga, gb
    w, v, al, a = tw[:3], tw[3:], ac[:3], ac[3:]
    gth, gp, gw, gv = a6[:3], a6[3:], b6[:3], b6[3:]
    a_o = a + np.cross(w, v)
    E, Jr, _, _ = sc.exp_and_right_jacobian(dt * w + h * al)
    d, vn = dt * v + h * a_o, E.T @ (v + dt * a_o)
    P, V = E @ gp, E @ gv
    s = Jr.T @ (gth + np.cross(gv, vn))
    gao = h * P + dt * V
    gq = np.concatenate([E @ gth + np.cross(d, P), P])
    gqd = np.concatenate([gw + dt * s + np.cross(v, gao), dt * P + V + np.cross(gao, w)])
    gqdd = np.concatenate([dt * gw + h * s, gao])
    return gq[sel], gqd[sel], gqdd[sel]
