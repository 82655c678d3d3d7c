"""CPU checker of mh_joint_limit_impulse_*: the projected Gauss-Seidel sweeps of include/mecano_hip.h restated in numpy, vectorised over
the batch, on S built from OracleModel.crba inverted densely -- nothing here walks the articulated-body recursion the device uses.  Per
configuration and listed joint i (DoF index d_i, configuration index c_i of the description's index maps)

    gap_lo = q[c_i] - lower_i, gap_hi = upper_i - q[c_i], s_i = +1 where gap_lo <= gap_hi else -1, gap_i = min(gap_lo, gap_hi),
    closed where gap_i <= margin,   b_i = s_i qd[d_i] + erp gap_i,   S_ij = s_i s_j Hinv[d_i][d_j] with its lower triangle mirrored,
    minimise 1/2 lam^T (S + eps I) lam + lam^T b  subject to lam >= 0 on the closed rows,   qd_next = qd + sum_closed (s_i lam_i) Hinv[:, d_i].

tests/test_joint_limits_cpu.py pins this file by facts not of its own making."""
import itertools

import numpy as np

DOFS = {0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}  # per joint type: revolute, prismatic, floating, fixed, planar, spherical
CFGS = {0: 1, 1: 1, 2: 7, 3: 0, 4: 3, 5: 4}


def joint_indices(desc, joints):
    """(d [L], c [L]): DoF and configuration index of every listed joint, which must be revolute or prismatic"""
    types = [int(t) for t in desc.joint_type]
    dofs = np.concatenate([[0], np.cumsum([DOFS[t] for t in types])])
    cfgs = np.concatenate([[0], np.cumsum([CFGS[t] for t in types])])
    di, ci = np.asarray(desc.dof_indices, dtype=np.int64).reshape(-1), np.asarray(desc.cfg_indices, dtype=np.int64).reshape(-1)
    for j in joints:
        assert types[j] in (0, 1), f"joint {j} is neither revolute nor prismatic"
    return np.array([di[dofs[j]] for j in joints]), np.array([ci[cfgs[j]] for j in joints])


def one_dof_joints(desc):
    return [j for j in range(desc.n_joints) if int(desc.joint_type[j]) in (0, 1)]


def rows(q, c, lower, upper, margin):
    """(s [B, L] of +-1, gap [B, L], closed [B, L])"""
    qc = np.asarray(q, dtype=float)[:, c]
    with np.errstate(invalid="ignore"):
        gap_lo, gap_hi = qc - np.asarray(lower, dtype=float)[None, :], np.asarray(upper, dtype=float)[None, :] - qc
        low = gap_lo <= gap_hi
        gap = np.where(low, gap_lo, gap_hi)
        return np.where(low, 1.0, -1.0), gap, gap <= margin


def objective(S, b, eps, lam):
    return 0.5 * np.einsum("bi,bij,bj->b", lam, S, lam) + 0.5 * eps * (lam * lam).sum(axis=1) + (lam * b).sum(axis=1)


def sweeps(S, b, closed, eps, iterations, lam0=None, history=None):
    """(lam [B, L], residual [B]): lam0 clamped at 0 on the closed rows, then `iterations` sweeps i = 0 ... L - 1 with the newest lam"""
    B, L = b.shape
    lam = np.zeros((B, L)) if lam0 is None else np.where(closed, np.maximum(0.0, lam0), 0.0)
    if history is not None:
        history.append(objective(S, b, eps, lam))
    res = np.zeros(B)
    for _ in range(iterations):
        res = np.zeros(B)
        for i in range(L):
            u = b[:, i] + np.einsum("bj,bj->b", S[:, i, :], lam) + eps * lam[:, i]
            new = np.where(closed[:, i], np.maximum(0.0, lam[:, i] - u / (S[:, i, i] + eps)), 0.0)
            res = np.maximum(res, np.abs(new - lam[:, i]))
            lam[:, i] = new
        if history is not None:
            history.append(objective(S, b, eps, lam))
    return lam, res


def terms(om, desc, q, qd, joints, lower, upper, margin, erp):
    """dict(H, Hinv, d, c, s, gap, closed, b, S)"""
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    d, c = joint_indices(desc, joints)
    H = om.crba(q)
    Hinv = np.linalg.inv(H)
    s, gap, closed = rows(q, c, lower, upper, margin)
    with np.errstate(invalid="ignore"):
        b = s * qd[:, d] + erp * gap
    block = Hinv[:, d][:, :, d]
    block = np.tril(block) + np.tril(block, -1).transpose(0, 2, 1)
    S = s[:, :, None] * block * s[:, None, :]
    return dict(H=H, Hinv=Hinv, d=d, c=c, s=s, gap=gap, closed=closed, b=b, S=S)


def stick_cond(H, d, closed, eps):
    """cond_inf of the KKT matrix [[H, E_c^T], [E_c, -eps I]] over the closed rows, per configuration (H alone where none is closed)"""
    B, nv = H.shape[:2]
    out = np.zeros(B)
    for r in range(B):
        on = d[closed[r]]
        m = len(on)
        K = np.zeros((nv + m, nv + m))
        K[:nv, :nv] = H[r]
        K[nv + np.arange(m), on] = 1.0
        K[on, nv + np.arange(m)] = 1.0
        K[nv:, nv:] = -eps * np.eye(m)
        out[r] = np.linalg.cond(K, np.inf)
    return out


def joint_limit_impulse(om, desc, q, qd, joints, lower, upper, margin=0.0, erp=0.0, compliance=0.0, iterations=50, init=None, history=None):
    """dict(qd_next [B, nv], impulse [B, L], residual [B], lam, cond_kkt, cond_H and the terms): what mh_joint_limit_impulse_* returns in
    AoS.  A configuration is NaN throughout where q of a listed joint is not finite, S_ii + eps of a closed row is not positive and
    finite, b or init of a closed row is not finite, or a lam after the last sweep is not finite."""
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    T = terms(om, desc, q, qd, joints, lower, upper, margin, erp)
    s, closed, S, b = T["s"], T["closed"], T["S"], T["b"]
    B, L = b.shape
    init = None if init is None else np.asarray(init, dtype=float).reshape(B, L)
    with np.errstate(invalid="ignore", divide="ignore"):
        lam, res = sweeps(np.where(np.isfinite(S), S, 0.0), np.where(closed, b, 0.0), closed, compliance, iterations, None if init is None else s * init, history)
        pivot = np.einsum("bii->bi", S) + compliance
    bad = ~np.isfinite(q[:, T["c"]]).all(axis=1) | (closed & ~(np.isfinite(pivot) & (pivot > 0))).any(axis=1) | (closed & ~np.isfinite(b)).any(axis=1)
    if init is not None:
        bad |= (closed & ~np.isfinite(init)).any(axis=1)
    bad |= ~np.isfinite(lam).all(axis=1)
    impulse = np.where(closed, s * lam, 0.0)
    qd_next = qd.copy()
    for i in range(L):
        qd_next += np.where(closed[:, i], impulse[:, i], 0.0)[:, None] * T["Hinv"][:, :, T["d"][i]]
    qd_next[bad], impulse[bad], res[bad], lam[bad] = np.nan, np.nan, np.nan, np.nan
    ok = ~bad
    cond_kkt, cond_H = np.full(B, np.nan), np.full(B, np.nan)
    cond_kkt[ok] = stick_cond(T["H"][ok], T["d"], closed[ok], compliance)
    cond_H[ok] = [np.linalg.cond(T["H"][r], np.inf) for r in np.nonzero(ok)[0]]
    return dict(T, qd_next=qd_next, impulse=impulse, residual=res, lam=lam, cond_kkt=cond_kkt, cond_H=cond_H, bad=bad)


def natural_residual(S, b, closed, eps, lam):
    """max_i |lam_i - max(0, lam_i - u_i)| over the closed rows (|lam_i| over the open ones), u = b + (S + eps I) lam: zero exactly at the solution"""
    u = b + np.einsum("bij,bj->bi", S, lam) + eps * lam
    return np.where(closed, np.abs(lam - np.maximum(0.0, lam - u)), np.abs(lam)).max(axis=1)


def exact(S, b, closed, eps):
    """lam [B, L] solving 0 <= lam _|_ (S + eps I) lam + b >= 0 on the closed rows by enumeration of the 2^m pressing sets (m <= 7); the
    matrix is positive definite: one set satisfies both signs, and rounding is settled by the least violation"""
    B, L = b.shape
    lam = np.zeros((B, L))
    for r in range(B):
        on = [i for i in range(L) if closed[r, i]]
        assert len(on) <= 7
        A = S[r] + eps * np.eye(L)
        best, best_x = np.inf, np.zeros(L)
        for size in range(len(on) + 1):
            for p in itertools.combinations(on, size):
                p = list(p)
                x = np.zeros(L)
                if p:
                    x[p] = np.linalg.solve(A[np.ix_(p, p)], -b[r, p])
                w = A @ x + b[r]
                viol = max([0.0] + [-x[i] for i in p] + [-w[i] for i in on if i not in p])
                if viol < best:
                    best, best_x = viol, x
        lam[r] = best_x
    return lam
