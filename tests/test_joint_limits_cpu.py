"""Pins of the CPU checker of the joint-limit impulses (tests/joint_limits_check.py) by facts not of its own making -- the complementarity
solution by enumeration of the pressing sets, a dense KKT solve of the rows that press, the descent of the objective, a mirror symmetry of
the arm's base joint -- and the case builders the device tests share.  No GPU."""
import numpy as np
import pytest

import joint_limits_check as jl
from helpers import U32, close_aba
from mecano_amd import random_tools as rt
from mecano_amd.multibody import MultiBodySystem, RigidBody
from oracle.cpu_oracle import OracleModel
from test_kinematics_cpu import make_case, states

LOWER, UPPER, MARGIN, ERP = -1.0, 1.0, 0.25, 50.0  # exact in fp32
THRESHOLDS = (LOWER + MARGIN, UPPER - MARGIN)      # where a row closes
B_CPU = 64
_MODELS = {}


COMB_CHAINS, COMB_DEPTH, COMB_SEED = 16, 4, 77


def comb16x4():
    """A fixed root body carrying 16 chains of 4 one-DoF joints, every fifth joint (in the order they are made, chain by chain) prismatic:
    64 rows that couple within a chain only, so that the stick system stays well conditioned at the cap of the list length
    (tests/test_joint_limits_wide_cpu.py pins how well).  The joint list is chain by chain: joint 4 c + k is joint k of chain c."""
    rng = np.random.default_rng(COMB_SEED)
    root = RigidBody("combBase")
    for c in range(COMB_CHAINS):
        body = root
        for k in range(COMB_DEPTH):
            make = rt.nextPrismaticJoint if (COMB_DEPTH * c + k) % 5 == 4 else rt.nextRevoluteJoint
            body = rt.nextRigidBody(rng, f"chain{c}Body{k}", make(rng, f"chain{c}Joint{k}", body))
    return MultiBodySystem.toMultiBodySystemInput(root)


def model_of(name):
    if name not in _MODELS:
        if name == "comb16x4":
            sys_ = comb16x4()
            desc = sys_.toModelDesc()
        else:
            sys_, desc = make_case(name)
        _MODELS[name] = (sys_, desc, OracleModel(desc))
    return _MODELS[name]


def make_inputs(name, B, seed=0, dtype=np.float64, joints=None):
    """dict(q, qd, joints, lower, upper, margin, erp): random states, every 1-DoF joint of the model listed (or `joints`) with the range
    +-1.  A q of a listed joint within 1e-3 of a closing threshold is moved 2e-3 away from it: raw states come as close as 1e-4, and a row
    must not open in one precision and close in the other.  Values are rounded to `dtype` and returned as fp64."""
    sys_, desc, om = model_of(name)
    joints = jl.one_dof_joints(desc) if joints is None else list(joints)
    q, qd = states(sys_, desc, B, seed=31 + seed)
    _, c = jl.joint_indices(desc, joints)
    for t in THRESHOLDS:
        near = np.abs(q[:, c] - t) < 1.0e-3
        q[:, c] = np.where(near, t + np.where(q[:, c] >= t, 2.0e-3, -2.0e-3), q[:, c])
    r = lambda x: np.asarray(x).astype(dtype).astype(np.float64)
    L = len(joints)
    return dict(q=r(q), qd=r(qd), joints=joints, lower=np.full(L, LOWER), upper=np.full(L, UPPER), margin=MARGIN, erp=ERP)


def solve(name, I, iterations, compliance=0.0, init=None, history=None, **over):
    _, desc, om = model_of(name)
    a = dict(I, **over)
    return jl.joint_limit_impulse(om, desc, a["q"], a["qd"], a["joints"], a["lower"], a["upper"], a["margin"], a["erp"], compliance, iterations, init, history)


_CONVERGED = {}


def converged(name):
    if name not in _CONVERGED:
        I = make_inputs(name, B_CPU)
        _CONVERGED[name] = (I, solve(name, I, 1000))
    return _CONVERGED[name]


@pytest.mark.parametrize("name,least", [("arm7", 2), ("humanoid30", 10)])
def test_inputs_are_what_they_claim(name, least):
    """69-77 % of the rows closed, at least 2 (10) per configuration, both sides, violated and merely near rows; cond(S_closed) ~ 1e2"""
    I, R = converged(name)
    share = R["closed"].mean()
    assert 0.69 <= share <= 0.77 and R["closed"].sum(axis=1).min() >= least, (share, R["closed"].sum(axis=1).min())
    assert (R["s"][R["closed"]] > 0).any() and (R["s"][R["closed"]] < 0).any()
    assert (R["gap"][R["closed"]] < 0).any() and (R["gap"][R["closed"]] > 0).any()
    assert np.abs(np.abs(I["q"][:, R["c"]]) - 0.75).min() >= 1.0e-3
    conds = [np.linalg.cond(R["S"][r][np.ix_(R["closed"][r], R["closed"][r])]) for r in range(B_CPU)]
    assert np.median(conds) < 1.0e3
    res200 = solve(name, I, 200)
    assert np.abs(res200["lam"] - R["lam"]).max() <= 1.0e-12 * max(1.0, np.abs(R["lam"]).max())  # 200 sweeps reach rounding level


def test_thousand_sweeps_are_the_enumerated_solution():
    I, R = converged("arm7")
    want = jl.exact(R["S"], R["b"], R["closed"], 0.0)
    scale = max(1.0, np.abs(want).max())
    assert np.abs(R["lam"] - want).max() <= 1.0e-9 * scale and np.abs(want).max() > 0.1
    assert jl.natural_residual(R["S"], R["b"], R["closed"], 0.0, R["lam"]).max() <= 1.0e-9 * scale
    assert (R["lam"] >= 0).all() and not R["lam"][~R["closed"]].any() and not R["impulse"][~R["closed"]].any()
    assert (R["s"] * R["impulse"] >= 0).all()


@pytest.mark.parametrize("name", ["arm7", "humanoid30"])
def test_the_objective_never_increases(name):
    I = make_inputs(name, B_CPU)
    rng = np.random.default_rng(3)
    for init in (None, rng.normal(size=(B_CPU, len(I["joints"])))):
        history = []
        solve(name, I, 30, 1.0e-6, init, history)
        h = np.array(history)
        assert len(h) == 31 and (np.diff(h, axis=0) <= 1.0e-12 * np.maximum(1.0, np.abs(h[:-1]))).all()
        assert (h[-1] < h[0]).any()


def test_a_row_that_leaves_gets_exactly_zero_and_all_open_returns_qd():
    name = "arm7"
    I = make_inputs(name, B_CPU)
    _, desc, om = model_of(name)
    d, c = jl.joint_indices(desc, I["joints"])
    s, gap, closed = jl.rows(I["q"], c, I["lower"], I["upper"], I["margin"])
    leaving = I["qd"].copy()
    leaving[:, d] = s * (1.0 + np.abs(leaving[:, d]))  # every row moves into its range; erp = 0: b = |qd| > 0 > -erp gap
    R = solve(name, I, 20, qd=leaving, erp=0.0)
    assert closed.any() and not R["impulse"].any() and np.array_equal(R["qd_next"], leaving) and not R["residual"].any()
    slow = I["qd"].copy()
    slow[:, d] = 0.0  # at rest: less than erp gap asks of a violated row -- listed alone, that row and no other gets an impulse
    R = solve(name, I, 20, qd=slow, joints=[3], lower=I["lower"][:1], upper=I["upper"][:1])
    violated = closed[:, 3] & (gap[:, 3] < 0.0)
    assert violated.any() and (R["lam"][violated, 0] > 0).all() and not R["lam"][~violated, 0].any()
    R = solve(name, I, 20, lower=np.full(7, -10.0), upper=np.full(7, 10.0))
    assert not R["closed"].any() and np.array_equal(R["qd_next"], I["qd"]) and not R["impulse"].any()
    R = solve(name, I, 20, lower=np.full(7, -np.inf), upper=np.full(7, np.inf))
    assert not R["closed"].any() and np.array_equal(R["qd_next"], I["qd"]) and not R["bad"].any()


def test_an_upper_row_mirrors_the_lower_row_of_minus_q():
    """The arm's inertia matrix does not depend on its base joint's angle: with that joint listed alone, (q0, qd0, [lo, hi]) and
    (-q0, -qd0, [-hi, -lo]) are mirror images -- the same lam, the opposite impulse and the opposite change of velocity."""
    name = "arm7"
    I = make_inputs(name, B_CPU, joints=[0])
    _, desc, om = model_of(name)
    d, c = jl.joint_indices(desc, [0])
    lo, hi = np.array([-0.9]), np.array([1.2])
    A = solve(name, I, 5, lower=lo, upper=hi)
    q, qd = I["q"].copy(), I["qd"].copy()
    q[:, c] *= -1.0
    qd[:, d] *= -1.0
    M = solve(name, I, 5, q=q, qd=qd, lower=-hi, upper=-lo)
    assert A["closed"].any() and (A["s"] > 0).any() and (A["s"] < 0).any()
    assert np.array_equal(A["s"], -M["s"]) and np.array_equal(A["closed"], M["closed"])
    scale = max(1.0, np.abs(A["impulse"]).max())
    assert np.abs(A["lam"] - M["lam"]).max() <= 1.0e-12 * scale and np.abs(A["impulse"] + M["impulse"]).max() <= 1.0e-12 * scale
    assert np.abs((A["qd_next"] - I["qd"]) + (M["qd_next"] - qd)).max() <= 1.0e-10 * scale


@pytest.mark.parametrize("name", ["arm7", "humanoid30"])
def test_pressing_rows_are_held_like_bilateral_constraints(name):
    """The rows that press are held as equalities in joint space, qd+[d_i] = -s_i erp gap_i -- the dense KKT system
    [[H, E^T], [E, 0]] (qd+, -impulse) = (H qd, -s erp gap) over them, solved here, gives the same velocity and impulses -- and the closed
    rows that do not press leave at least as fast as asked.  In some configurations every closed row presses."""
    I, R = converged(name)
    nv = R["H"].shape[1]
    pressing = R["lam"] > 1.0e-9
    assert sum((pressing[r] == R["closed"][r]).all() for r in range(B_CPU)) >= (3 if name == "arm7" else 0) and (pressing != R["closed"]).any()
    for r in range(B_CPU):
        on = np.nonzero(pressing[r])[0]
        idle = np.nonzero(R["closed"][r] & ~pressing[r])[0]
        assert (R["s"][r, idle] * R["qd_next"][r, R["d"][idle]] + ERP * R["gap"][r, idle] >= -1.0e-9).all()
        dd, m = R["d"][on], len(on)
        K = np.zeros((nv + m, nv + m))
        K[:nv, :nv] = R["H"][r]
        K[nv + np.arange(m), dd] = 1.0
        K[dd, nv + np.arange(m)] = 1.0
        x = np.linalg.solve(K, np.concatenate([R["H"][r] @ I["qd"][r], -R["s"][r, on] * ERP * R["gap"][r, on]]))
        scale = max(1.0, np.abs(x).max())
        assert np.abs(x[:nv] - R["qd_next"][r]).max() <= 1.0e-8 * scale and np.abs(-x[nv:] - R["impulse"][r, on]).max() <= 1.0e-8 * scale
        assert np.abs(R["s"][r, on] * R["qd_next"][r, dd] + ERP * R["gap"][r, on]).max() <= 1.0e-9 * scale


def test_a_bad_configuration_is_nan_throughout():
    name = "arm7"
    I = make_inputs(name, 8)
    _, desc, om = model_of(name)
    d, c = jl.joint_indices(desc, I["joints"])
    good = solve(name, I, 5)
    q, qd, init = I["q"].copy(), I["qd"].copy(), np.zeros((8, 7))
    q[1, c[2]] = np.nan
    row = int(np.nonzero(good["closed"][3])[0][0])
    qd[3, d[row]] = np.nan
    init[5, int(np.nonzero(good["closed"][5])[0][0])] = np.nan
    R = solve(name, I, 5, init=init, q=q, qd=qd)
    assert R["bad"].tolist() == [False, True, False, True, False, True, False, False]
    for k in ("qd_next", "impulse", "residual"):
        assert np.isnan(R[k][[1, 3, 5]]).all() and np.array_equal(R[k][[0, 2, 4, 6, 7]], good[k][[0, 2, 4, 6, 7]])


def planted(name, I, fault, iterations=50):
    """The checker's result with one mistake a kernel could make"""
    _, desc, om = model_of(name)
    T = jl.terms(om, desc, I["q"], I["qd"], I["joints"], I["lower"], I["upper"], I["margin"], I["erp"])
    s, closed, d = T["s"], T["closed"], T["d"]
    block = T["Hinv"][:, d][:, :, d]
    block = np.tril(block) + np.tril(block, -1).transpose(0, 2, 1)
    S = T["S"]
    if fault == "column sign":
        S = s[:, :, None] * block
    elif fault == "triangle not mirrored":
        S = s[:, :, None] * np.tril(T["Hinv"][:, d][:, :, d]) * s[:, None, :]
    lam0 = s * I["init"]
    lam, _ = jl.sweeps(S, T["b"], closed, 0.0, iterations, lam0)
    if fault == "open rows kept":  # the warm start survives on an open row and is summed
        lam = np.where(closed, lam, np.maximum(0.0, lam0))
    impulse = lam if fault == "upper pushes up" else s * lam
    if fault != "open rows kept":
        impulse = np.where(closed, impulse, 0.0)
    qd_next = I["qd"] + np.einsum("bi,bri->br", impulse, T["Hinv"][:, :, d])
    return qd_next, impulse


@pytest.mark.parametrize("fault", ["none", "column sign", "triangle not mirrored", "upper pushes up", "open rows kept"])
def test_planted_faults_are_rejected(fault):
    """The comparison the device tests make -- close_aba on (qd+, impulse) with the stick system's cond_inf, here at the fp32 unit
    roundoff, the wider of the two -- passes the checker's own result and rejects each mistake."""
    name = "arm7"
    I = make_inputs(name, B_CPU)
    I["init"] = np.random.default_rng(9).normal(size=(B_CPU, 7))
    _, desc, om = model_of(name)
    R = solve(name, I, 50, init=I["init"])
    v, p = planted(name, I, fault)
    got, want = np.concatenate([v, p], axis=1), np.concatenate([R["qd_next"], R["impulse"]], axis=1)
    if fault == "none":
        close_aba(got, want, None, desc.n_joints, U32, label="checker against itself", conds=R["cond_kkt"])
        return
    with pytest.raises(AssertionError):
        close_aba(got, want, None, desc.n_joints, U32, label=None, conds=R["cond_kkt"])
