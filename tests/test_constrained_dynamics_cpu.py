"""Pins of the CPU checker of the constrained dynamics (tests/constrained_dynamics_check.py) by facts not of its own making -- the C oracle's
forward dynamics under the wrenches it reports, the unconstrained limit, the duplicate-target identity, the constraint equation itself --
and the case builders the device tests share.  No GPU."""
import zlib

import numpy as np
import pytest

import constrained_dynamics_check as cc
import kinematics_check as kc
from helpers import close
from oracle.cpu_oracle import OracleModel
from test_kinematics_cpu import HUMANOID_TARGETS, make_case, states

# name -> (model of test_kinematics_cpu.make_case, targets, row masks): m = 12, 3, 6, 8, 8 rows
CASES = {
    "humanoid30": ("humanoid30", HUMANOID_TARGETS, [cc.POINT, cc.POINT, cc.WELD, 0]),  # feet as points, one hand welded, one hand free
    "arm7_point": ("arm7", [6], [cc.POINT]),
    "arm7_weld": ("arm7", [6], [cc.WELD]),
    "onedof12": ("onedof12", [3, 7, 11], [0b111000, 0b000111, 0b100100]),
    "mixed12": ("mixed12", [3, 7, 11], [0b111000, 0b000111, 0b100100]),
}
GRAVITY = (0.3, -0.2, -9.81)
_MODELS = {}


def model_of(name):
    """(system, desc, OracleModel) of a case, built once"""
    key = CASES[name][0]
    if key not in _MODELS:
        sys_, desc = make_case(key)
        _MODELS[key] = (sys_, desc, OracleModel(desc))
    return _MODELS[key]


def random_active(rng, B, rows):
    """[B, K] int32: about a quarter of the rows off, bits outside the row masks set at random (they are ignored), and every eighth
    configuration (from the third on) with no row active at all."""
    K = len(rows)
    act = np.zeros((B, K), dtype=np.int32)
    for k in range(K):
        bits = rng.random((B, 6)) < 0.75
        act[:, k] = (bits * (1 << np.arange(6))).sum(axis=1)
    act[2::8] = 0
    for k, rk in enumerate(rows):  # a bit outside the mask must change nothing: set those of every other configuration
        act[::2, k] |= 0x3F & ~int(rk)
    return act


def make_inputs(name, B, seed=0, dtype=np.float64, with_active=True):
    """Everything a call takes, in AoS: dict(desc, q, qd, tau, f_ext, targets, rows, poses, active, a_des, v_des).  Values are rounded to
    `dtype` and returned as fp64 (what the device holds in that precision)."""
    sys_, desc, _ = model_of(name)
    _, targets, rows = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 101 * seed)
    q, qd = states(sys_, desc, B, seed=17 + seed)
    K = len(targets)
    r = lambda x: np.asarray(x).astype(dtype).astype(np.float64)
    return dict(desc=desc, q=r(q), qd=r(qd), tau=r(rng.uniform(-5.0, 5.0, (B, desc.nv))), f_ext=r(rng.uniform(-2.0, 2.0, (B, desc.n_joints, 6))),
                targets=list(targets), rows=list(rows), poses=kc.random_poses(rng, K), active=random_active(rng, B, rows) if with_active else None,
                a_des=r(rng.uniform(-1.0, 1.0, (B, K, 6))), v_des=r(rng.uniform(-0.5, 0.5, (B, K, 6))))


def reference(name, I, compliance=0.0):
    _, desc, om = model_of(name)
    return cc.aba_constrained(om, desc, I["q"], I["qd"], I["tau"], I["targets"], I["rows"], I["poses"], I["active"], I["a_des"], compliance, GRAVITY,
                              I["f_ext"])


def reference_impulse(name, I, compliance=0.0):
    _, desc, om = model_of(name)
    return cc.constraint_impulse(om, desc, I["q"], I["qd"], I["targets"], I["rows"], I["poses"], I["active"], I["v_des"], compliance)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_forward_dynamics_under_the_reported_wrenches_reproduces_qdd(name):
    """qdd of the KKT system is OracleModel.aba of the same state with f_ext + sum X_k^T lambda_k: signs, frames and the row selection."""
    _, desc, om = model_of(name)
    I = make_inputs(name, 6)
    R = reference(name, I)
    print(f"{name}: cond_inf(KKT) <= {R['cond_kkt'].max():.2e}, cond_inf(H) <= {R['cond_H'].max():.2e}")
    f = cc.wrenches_on_bodies(desc, I["targets"], I["poses"], R["lam"], I["f_ext"])
    qdd = om.aba(I["q"], I["qd"], I["tau"], GRAVITY, f)
    tol = 1.0e-15 * R["cond_kkt"].max() * 64  # both sides solve with this matrix's conditioning
    close(qdd, R["qdd"], max(tol, 1.0e-11), label=name)
    assert np.abs(R["lam"]).max() > 0.1
    for r in range(6):  # rows that take no part hold exactly zero
        s = cc.selected_rows(I["rows"], I["active"][r])
        off = np.setdiff1d(np.arange(6 * len(I["targets"])), s)
        assert not R["lam"][r].reshape(-1)[off].any()


@pytest.mark.parametrize("name", ["humanoid30", "mixed12"])
def test_all_rows_inactive_is_the_free_forward_dynamics(name):
    _, desc, om = model_of(name)
    I = make_inputs(name, 3)
    I["active"] = np.zeros_like(I["active"])
    R = reference(name, I)
    assert not R["lam"].any()
    close(R["qdd"], om.aba(I["q"], I["qd"], I["tau"], GRAVITY, I["f_ext"]), 1.0e-15 * R["cond_H"].max() * 64, label=name)


def test_root_acceleration_enters_through_the_dynamics_only():
    """A 6-D root acceleration in place of gravity: the constraint is on the motion relative to the root, so only h changes."""
    name = "arm7_weld"
    _, desc, om = model_of(name)
    I = make_inputs(name, 3, with_active=False)
    root = (0.4, -0.3, 0.2, 1.0, -2.0, 9.0)
    R = cc.aba_constrained(om, desc, I["q"], I["qd"], I["tau"], I["targets"], I["rows"], I["poses"], None, I["a_des"], 0.0, root, I["f_ext"])
    f = cc.wrenches_on_bodies(desc, I["targets"], I["poses"], R["lam"], I["f_ext"])
    close(om.aba(I["q"], I["qd"], I["tau"], root, f), R["qdd"], 1.0e-11, label="root acceleration")


def duplicate_compliance(name="humanoid30", B=4):
    """(eps, worst cond_inf) for the duplicate-target identity, W the 3 x 3 linear block of the left foot: the smallest power of ten for
    which the doubled matrix [[W + eps I, W], [W, W + eps I]] stays under 1e4 -- it decides how well the even split of lambda is determined
    (its smallest eigenvalue is eps) -- and with it cond_inf(2 W + eps I) of the single constraint it is compared with."""
    _, desc, om = model_of(name)
    I = make_inputs(name, B, seed=3, with_active=False)
    Jt, _ = kc.geometric_jacobian(kc.KinModel(desc), I["q"], [6], None, I["poses"][:1])
    H = om.crba(I["q"])
    W = np.stack([Jt[r][3:] @ np.linalg.solve(H[r], Jt[r][3:].T) for r in range(B)])
    for e in range(-8, 1):
        eps = 10.0 ** e
        worst = max(max(np.linalg.cond(2 * W[r] + eps * np.eye(3), np.inf),
                        np.linalg.cond(np.block([[W[r] + eps * np.eye(3), W[r]], [W[r], W[r] + eps * np.eye(3)]]), np.inf)) for r in range(B))
        if worst < 1.0e4:
            return eps, worst
    raise AssertionError("no compliance under 1e4")


def test_duplicated_target_splits_lambda_and_halves_the_compliance():
    """Two identical point constraints with compliance eps: lambda split evenly, qdd that of the single constraint with eps / 2.  Without
    compliance the doubled rows are singular."""
    name = "humanoid30"
    _, desc, om = model_of(name)
    eps, cond = duplicate_compliance()
    print(f"eps = {eps:g}: cond_inf(2 W + eps I) and cond_inf of the doubled matrix <= {cond:.2e}")
    I = make_inputs(name, 4, seed=3, with_active=False)
    pose, a = I["poses"][:1], I["a_des"][:, :1]
    args = (om, desc, I["q"], I["qd"], I["tau"])
    two = cc.aba_constrained(*args, [6, 6], [cc.POINT, cc.POINT], np.tile(pose, (2, 1)), None, np.tile(a, (1, 2, 1)), eps, GRAVITY, I["f_ext"])
    one = cc.aba_constrained(*args, [6], [cc.POINT], pose, None, a, eps / 2, GRAVITY, I["f_ext"])
    close(two["qdd"], one["qdd"], 1.0e-10, label="qdd")
    close(two["lam"][:, 0], 0.5 * one["lam"][:, 0], 1.0e-10, label="lambda 0")
    close(two["lam"][:, 1], 0.5 * one["lam"][:, 0], 1.0e-10, label="lambda 1")
    J2, _ = kc.geometric_jacobian(kc.KinModel(desc), I["q"][:1], [6, 6], None, np.tile(pose, (2, 1)))
    Jc = J2[0][cc.selected_rows([cc.POINT, cc.POINT])]
    assert np.linalg.matrix_rank(Jc) == 3  # six rows of rank three: singular without compliance (cond > 1e16)


def test_arm_weld_with_a_des_cancelling_c_keeps_J_qdd_zero():
    """The defining equation is J_c qdd + c + eps lambda = a_des, c = Jdot qd: with a_des = c the welded frame has J_c qdd = 0, with a_des = 0
    it has J_c qdd = -c (the frame's relative acceleration vanishes), with a_des = -c it has J_c qdd = -2 c."""
    name = "arm7_weld"
    _, desc, om = model_of(name)
    I = make_inputs(name, 4, with_active=False)
    J, c = kc.geometric_jacobian(kc.KinModel(desc), I["q"], I["targets"], None, I["poses"], I["qd"])
    c = c.reshape(4, 6)
    assert np.abs(c).max() > 0.1
    for factor in (1.0, 0.0, -1.0):
        R = cc.aba_constrained(om, desc, I["q"], I["qd"], I["tau"], I["targets"], I["rows"], I["poses"], None, factor * c, 0.0, GRAVITY, I["f_ext"])
        close(np.einsum("bij,bj->bi", J, R["qdd"]), (factor - 1.0) * c, 1.0e-15 * R["cond_kkt"].max() * 64, absolute=True, label=f"J qdd, a_des = {factor} c")
        assert np.abs(R["qdd"]).max() > 0.1


@pytest.mark.parametrize("name", ["humanoid30", "onedof12"])
def test_impulse_leaves_a_velocity_that_meets_v_des_alone(name):
    _, desc, om = model_of(name)
    I = make_inputs(name, 4)
    J, _ = kc.geometric_jacobian(kc.KinModel(desc), I["q"], I["targets"], None, I["poses"])
    I["v_des"] = np.einsum("bij,bj->bi", J, I["qd"]).reshape(4, -1, 6)
    R = reference_impulse(name, I)
    close(R["qd_next"], I["qd"], 1.0e-15 * R["cond_kkt"].max() * 64, label="qd unchanged")
    close(R["impulse"], np.zeros_like(R["impulse"]), 1.0e-15 * R["cond_kkt"].max() * 64, absolute=True, label="no impulse")
    I["v_des"] = None  # the frames stop: the selected rows of J qd+ vanish, and the change is H^-1 J^T Lambda, the oracle's zero-velocity dynamics
    R = reference_impulse(name, I)
    assert cc.constraint_residual(R, I["rows"], I["active"], R["qd_next"], R["impulse"], None, 0.0).max() <= 1.0e-15 * R["cond_kkt"].max() * 64
    f = cc.wrenches_on_bodies(desc, I["targets"], I["poses"], R["impulse"])
    z = np.zeros_like(I["qd"])
    close(om.aba(I["q"], z, z, (0.0, 0.0, 0.0), f), R["qd_next"] - I["qd"], 1.0e-15 * R["cond_kkt"].max() * 64, label="propagation")


def test_case_conditioning_is_reported():
    """cond_inf of the matrices the device tests' bound is built on, printed for the record (pytest -s)."""
    for name in CASES:
        R = reference(name, make_inputs(name, 16))
        print(f"{name}: m = {len(cc.selected_rows(CASES[name][2]))}, cond_inf(KKT) {R['cond_kkt'].min():.1e} .. {R['cond_kkt'].max():.1e}, "
              f"cond_inf(H) <= {R['cond_H'].max():.1e}")
        assert np.isfinite(R["cond_kkt"]).all()
