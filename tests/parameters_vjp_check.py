"""CPU checker of mh_rnea_parameters_vjp_* / mh_aba_parameters_vjp_*: the gradients of the inverse and the forward dynamics with respect
to the ten inertial numbers per body of every row, from the oracle's regressor (tests/inertial_parameters_check.py:
first_moment_regressor, the derivative with respect to (m, m c, J), which does not depend on the parameters) and the chain rule to
(m, c, J) with the row's own parameters.  The forward form takes qdd and H from the row's own OracleModel and mu = H^-1 w from a dense
solve.  tests/test_parameters_vjp_cpu.py pins both by central differences of Checker.rnea / Checker.aba."""
import numpy as np

import inertial_parameters_check as ipc


def chain(pi, ghat):
    """[..., n, 10] gradient with respect to (m, c, J) from the one with respect to (m, h = m c, J), at the parameters pi."""
    pi, ghat = np.asarray(pi, dtype=np.float64), np.asarray(ghat, dtype=np.float64)
    g = ghat.copy()
    g[..., 0] = ghat[..., 0] + (pi[..., 1:4] * ghat[..., 1:4]).sum(-1)
    g[..., 1:4] = pi[..., 0:1] * ghat[..., 1:4]
    return g


def amplification(pi):
    """chi per row: max over the bodies of max(1, m, 1 + |c|_1), what the chain rule multiplies an error of the regressor's columns by."""
    pi = np.asarray(pi, dtype=np.float64)
    return np.maximum(1.0, np.maximum(np.abs(pi[..., 0]), 1.0 + np.abs(pi[..., 1:4]).sum(-1))).max(axis=-1)


def _rows(B, rows):
    return np.arange(B) if rows is None else np.asarray(rows)


def rnea_parameters_vjp(desc, q, qd, qdd, pi, u, gravity, consider_coriolis=True, consider_accelerations=True, rows=None):
    """(g [B, n, 10], |Y|_inf [B], chi [B]) with g[r] = chain(Y(q_r, qd_r, qdd_r)^T u_r) at pi[r].  A switch that is off is that input at
    zero (Checker.rnea: the oracle's own Coriolis switch takes bodies with an offset centre of mass down another branch).  rows: the rows
    to evaluate; the others stay zero (scale and chi one)."""
    B, n = q.shape[0], desc.n_joints
    pi = np.asarray(pi, dtype=np.float64).reshape(B, n, 10)
    at = _rows(B, rows)
    qd = qd if consider_coriolis else np.zeros((B, desc.nv))
    qdd = qdd if consider_accelerations else np.zeros((B, desc.nv))
    Y = ipc.first_moment_regressor(desc, q[at], qd[at], qdd[at], gravity)
    g, scale, chi = np.zeros((B, n, 10)), np.ones(B), np.ones(B)
    g[at] = chain(pi[at], np.einsum("bi,bij->bj", u[at], Y).reshape(len(at), n, 10))
    scale[at] = np.abs(Y).reshape(len(at), -1).max(axis=1) if Y.size else 0.0
    chi[at] = amplification(pi[at])
    return g, scale, chi


def aba_parameters_vjp(desc, q, qd, tau, pi, w, gravity, f_ext=None, rows=None, checker=None):
    """(qdd [B, nv], mu [B, nv], g [B, n, 10], |H^-1 Y|_inf [B], chi [B], cond_inf(H) [B]): qdd and H of row r from the row's own
    OracleModel, mu = H^-1 w by a dense solve, g = -chain(Y(q, qd, qdd)^T mu) at pi[r]."""
    B, n, nv = q.shape[0], desc.n_joints, desc.nv
    pi = np.asarray(pi, dtype=np.float64).reshape(B, n, 10)
    at = _rows(B, rows)
    ck = checker or ipc.Checker(desc)
    qdd, mu, H = np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv, nv))
    for r in at:
        om = ck.model(pi[r])
        qdd[r] = om.aba(q[r:r + 1], qd[r:r + 1], tau[r:r + 1], gravity, None if f_ext is None else np.asarray(f_ext)[r:r + 1])[0]
        H[r] = om.crba(q[r:r + 1])[0]
        mu[r] = np.linalg.solve(H[r], w[r])
    Y = ipc.first_moment_regressor(desc, q[at], qd[at], qdd[at], gravity)
    g, scale, chi, conds = np.zeros((B, n, 10)), np.ones(B), np.ones(B), np.ones(B)
    g[at] = -chain(pi[at], np.einsum("bi,bij->bj", mu[at], Y).reshape(len(at), n, 10))
    for k, r in enumerate(at):
        scale[r] = np.abs(np.linalg.solve(H[r], Y[k])).max()
        conds[r] = np.linalg.cond(H[r], np.inf)
    chi[at] = amplification(pi[at])
    return qdd, mu, g, scale, chi, conds
