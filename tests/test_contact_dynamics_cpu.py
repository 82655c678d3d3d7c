"""Pins of the CPU checker of the frictional contact impulses (tests/contact_dynamics_check.py) by facts not of its own making -- the
frictionless solution by enumeration of the pressing sets, the stick solution of the dense KKT checker, the cone and the optimality
residual -- and the case builders the device tests share.  No GPU."""
import zlib

import numpy as np
import pytest

import constrained_dynamics_check as cc
import contact_dynamics_check as cd
import kinematics_check as kc
from oracle.cpu_oracle import OracleModel
from test_kinematics_cpu import HUMANOID_TARGETS, make_case, states

# name -> (model of test_kinematics_cpu.make_case, targets, compliance).  humanoid30_k8: four corners under each foot, twelve rows of rank
# six per foot -- S is singular and the compliance carries the solve
CASES = {
    "arm7": ("arm7", [6], 0.0),
    "humanoid30": ("humanoid30", HUMANOID_TARGETS, 0.0),
    "humanoid30_k8": ("humanoid30", [6, 6, 6, 6, 12, 12, 12, 12], 1.0e-6),
}
CPU_CASES = ["arm7", "humanoid30"]
B_CPU = 64
_MODELS = {}


def model_of(name):
    key = CASES[name][0]
    if key not in _MODELS:
        sys_, desc = make_case(key)
        _MODELS[key] = (sys_, desc, OracleModel(desc))
    return _MODELS[key]


def corner_poses(K):
    """identity rotations, the corners of a 0.2 m x 0.1 m sole 0.05 m below the body-fixed frame, four per body"""
    out = np.tile(kc.IDENTITY12, (K, 1))
    for k in range(K):
        out[k, 9:] = (0.1 if k & 1 else -0.1, 0.05 if k & 2 else -0.05, -0.05)
    return out


def make_inputs(name, B, seed=0, dtype=np.float64):
    """Everything a call takes, in AoS: dict(q, qd, targets, poses, normals, active, v_normal, compliance).  Random unit normals; the free
    velocity is the random one shifted (least change of qd) so that every contact approaches at 1 m/s along its normal.  active: about a
    quarter off; v_normal: uniform in +-0.3.  Values are rounded to `dtype` and returned as fp64."""
    sys_, desc, om = model_of(name)
    _, targets, eps = CASES[name]
    K = len(targets)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 977 * seed)
    q, qd = states(sys_, desc, B, seed=23 + seed)
    poses = corner_poses(K) if name.endswith("k8") else kc.random_poses(rng, K)
    normals = rng.normal(size=(B, K, 3))
    normals /= np.linalg.norm(normals, axis=2, keepdims=True)
    r = lambda x: np.asarray(x).astype(dtype).astype(np.float64)
    q, normals = r(q), r(normals)
    T = cd.terms(om, desc, q, qd, targets, poses, normals)
    Jn = np.einsum("bki,bkij->bkj", T["n"], T["Jl"].reshape(B, K, 3, -1))
    for row in range(B):
        qd[row] += np.linalg.pinv(Jn[row]) @ (-1.0 - Jn[row] @ qd[row])
    return dict(q=q, qd=r(qd), targets=list(targets), poses=poses, normals=normals, active=(rng.random((B, K)) < 0.75).astype(np.int32),
                v_normal=r(rng.uniform(-0.3, 0.3, (B, K))), compliance=eps)


def solve(name, I, mu, iterations, active=None, v_normal=None, init=None, history=None, precision=None):
    _, desc, om = model_of(name)
    K = len(I["targets"])
    return cd.contact_impulse(om, desc, I["q"], I["qd"], I["targets"], [mu] * K if np.isscalar(mu) else mu, I["poses"], I["normals"], active, v_normal,
                              I["compliance"], iterations, init, history, precision)


_CONVERGED = {}


def converged(name, mu):
    """(inputs, result of 1000 sweeps with every contact closed and v_normal = 0), once per (case, mu)"""
    if (name, mu) not in _CONVERGED:
        I = make_inputs(name, B_CPU)
        _CONVERGED[(name, mu)] = (I, solve(name, I, mu, 1000))
    return _CONVERGED[(name, mu)]


def lam_of(R):
    return R["impulse"][:, :, 3:]


@pytest.mark.parametrize("name", CPU_CASES)
def test_inputs_are_what_they_claim(name):
    I, R = converged(name, 0.5)
    K = len(I["targets"])
    un = np.einsum("bki,bki->bk", R["n"], R["b"].reshape(B_CPU, K, 3))
    assert np.abs(un + 1.0).max() < 1.0e-9  # every contact approaches at 1 m/s
    assert np.abs(np.linalg.norm(R["n"], axis=2) - 1.0).max() < 1.0e-12
    conds = np.array([np.linalg.cond(R["S"][r]) for r in range(B_CPU)])
    print(f"{name}: cond(S) {conds.min():.2f} .. {conds.max():.2f}")
    assert np.array_equal(R["S"], R["S"].transpose(0, 2, 1))  # exactly symmetric
    assert not R["impulse"][:, :, :3].any()


@pytest.mark.parametrize("name", CPU_CASES)
def test_frictionless_equals_the_enumerated_complementarity_solution(name):
    I, R = converged(name, 0.0)
    want = cd.frictionless_exact(R["S"], R["b"], R["n"], None, I["compliance"])
    scale = max(1.0, np.abs(want).max())
    err = np.abs(lam_of(R) - want).max()
    print(f"{name}: |lam - exact| = {err:.2e}, |lam| <= {scale:.2f}, natural residual {cd.natural_residual(R['S'], R['b'], R['n'], [0.0] * len(I['targets']), None, I['compliance'], lam_of(R)).max():.2e}")
    assert err <= 1.0e-10 * scale
    assert np.abs(want).max() > 0.1
    # complementarity through the checker's own terms: 0 <= n.lam, n.u+ >= 0, one of them zero
    K = len(I["targets"])
    ln = np.einsum("bki,bki->bk", R["n"], lam_of(R))
    up = (R["b"] + np.einsum("bij,bj->bi", R["S"], lam_of(R).reshape(B_CPU, -1))).reshape(B_CPU, K, 3)
    un = np.einsum("bki,bki->bk", R["n"], up) + I["compliance"] * ln
    assert ln.min() >= 0.0 and un.min() >= -1.0e-10 * scale and np.abs(ln * un).max() <= 1.0e-10 * scale


@pytest.mark.parametrize("name", CPU_CASES)
def test_stick_inside_the_cone_is_the_bilateral_solution(name):
    mu = 100.0
    I, R = converged(name, mu)
    _, desc, om = model_of(name)
    K = len(I["targets"])
    stick = cc.constraint_impulse(om, desc, I["q"], I["qd"], I["targets"], [cc.POINT] * K, I["poses"], None, None, I["compliance"])
    ls = stick["impulse"][:, :, 3:]
    sn = np.einsum("bki,bki->bk", R["n"], ls)
    st = np.linalg.norm(ls - sn[:, :, None] * R["n"], axis=2)
    inside = ((sn > 0) & (st <= 0.9 * mu * sn)).all(axis=1)  # with margin: a tenth of the cone's opening
    print(f"{name}: {inside.sum()} of {B_CPU} stick solutions lie inside their cones")
    assert inside.sum() * 2 >= B_CPU
    scale = max(1.0, np.abs(ls[inside]).max())
    assert np.abs(lam_of(R)[inside] - ls[inside]).max() <= 1.0e-9 * scale
    assert np.abs(R["qd_next"][inside] - stick["qd_next"][inside]).max() <= 1.0e-9 * max(1.0, np.abs(stick["qd_next"]).max())


@pytest.mark.parametrize("name", CPU_CASES)
def test_sliding_contacts_sit_on_the_cone_and_the_solution_is_optimal(name):
    mu = 0.5
    I, R = converged(name, mu)
    K = len(I["targets"])
    lam = lam_of(R)
    scale = max(1.0, np.abs(lam).max())
    nat = cd.natural_residual(R["S"], R["b"], R["n"], [mu] * K, None, I["compliance"], lam).max()
    print(f"{name}: natural residual {nat:.2e} at 1000 sweeps, |lam| <= {scale:.2f}, "
          f"{cd.natural_residual(R['S'], R['b'], R['n'], [mu] * K, None, I['compliance'], lam_of(solve(name, I, mu, 200))).max():.2e} at 200")
    assert nat <= 1.0e-12 * scale
    ln = np.einsum("bki,bki->bk", R["n"], lam)
    lt = np.linalg.norm(lam - ln[:, :, None] * R["n"], axis=2)
    assert ln.min() >= 0.0 and (lt <= mu * ln * (1.0 + 1.0e-12) + 1.0e-14).all()  # inside the cone
    up = (R["b"] + np.einsum("bij,bj->bi", R["S"], lam.reshape(B_CPU, -1)) + I["compliance"] * lam.reshape(B_CPU, -1)).reshape(B_CPU, K, 3)
    ut = up - np.einsum("bki,bki->bk", R["n"], up)[:, :, None] * R["n"]
    sliding = (np.linalg.norm(ut, axis=2) > 1.0e-6) & (ln > 1.0e-6)
    assert sliding.any()
    assert np.abs(lt[sliding] - mu * ln[sliding]).max() <= 1.0e-10 * scale  # on the cone ...
    tl = lam - ln[:, :, None] * R["n"]
    cosine = np.einsum("bki,bki->bk", tl, ut)[sliding] / (lt[sliding] * np.linalg.norm(ut, axis=2)[sliding])
    assert cosine.max() <= -1.0 + 1.0e-8  # ... opposed to the tangential velocity


@pytest.mark.parametrize("mu", [0.0, 0.5, 100.0])
@pytest.mark.parametrize("name", CPU_CASES)
def test_objective_never_increases(name, mu):
    I = make_inputs(name, B_CPU)
    hist = []
    rng = np.random.default_rng(3)
    init = np.zeros((B_CPU, len(I["targets"]), 6))
    init[:, :, 3:] = rng.normal(size=(B_CPU, len(I["targets"]), 3)) * 5.0  # a stale warm start, outside the cones
    solve(name, I, mu, 60, init=init, history=hist)
    h = np.array(hist)
    assert (h[1:] <= h[:-1] + 1.0e-13 * np.maximum(1.0, np.abs(h[:-1]))).all()
    assert (h[-1] < h[0]).all()


@pytest.mark.parametrize("name", CPU_CASES)
def test_a_contact_that_separates_faster_than_v_normal_gets_exactly_zero(name):
    """One contact leaving along its normal at 2 m/s with v_normal = 0.5: -rho b lies in the polar cone, the projection is the origin
    from the first sweep on.  (With a large tangential velocity the relaxation does pull on a separating contact: the cone admits an
    impulse that lowers the objective.  That is the model, and why the free velocity here is along the normal.)"""
    I = make_inputs(name, B_CPU)
    _, desc, om = model_of(name)
    tgt, pose, nh = I["targets"][:1], I["poses"][:1], I["normals"][:, :1]
    T = cd.terms(om, desc, I["q"], I["qd"], tgt, pose, nh)
    qd = I["qd"].copy()
    for row in range(B_CPU):
        qd[row] += np.linalg.pinv(T["Jl"][row]) @ (2.0 * T["n"][row, 0] - T["Jl"][row] @ qd[row])
    v = np.full((B_CPU, 1), 0.5)
    for mu in (0.0, 0.5):
        R = cd.contact_impulse(om, desc, I["q"], qd, tgt, [mu], pose, nh, None, v, 0.0, 50)
        assert not R["impulse"].any() and np.array_equal(R["qd_next"], qd) and not R["residual"].any()
    R = cd.contact_impulse(om, desc, I["q"], qd, tgt, [0.5], pose, nh, None, np.full((B_CPU, 1), 2.5), 0.0, 50)
    assert (np.einsum("bi,bi->b", R["impulse"][:, 0, 3:], T["n"][:, 0]) > 0.1).all()  # asked to leave faster than it does: it is pushed


@pytest.mark.parametrize("name", CPU_CASES)
def test_inactive_contacts_are_exactly_zero_and_the_rest_is_the_call_without_them(name):
    I = make_inputs(name, B_CPU)
    K = len(I["targets"])
    act = I["active"].copy()
    act[:, 0] = 0 if K > 1 else act[:, 0]
    R = solve(name, I, 0.5, 80, active=act, v_normal=I["v_normal"])
    assert not R["impulse"][act == 0].any()
    assert (act == 0).any() and R["impulse"][act != 0].any()
    if K > 1:  # contact 0 is open everywhere: the call on the other contacts alone
        _, desc, om = model_of(name)
        sub = cd.contact_impulse(om, desc, I["q"], I["qd"], I["targets"][1:], [0.5] * (K - 1), I["poses"][1:], I["normals"][:, 1:], act[:, 1:],
                                 I["v_normal"][:, 1:], I["compliance"], 80)
        assert np.abs(R["impulse"][:, 1:] - sub["impulse"]).max() <= 1.0e-13 * max(1.0, np.abs(sub["impulse"]).max())
        assert np.abs(R["qd_next"] - sub["qd_next"]).max() <= 1.0e-13 * max(1.0, np.abs(sub["qd_next"]).max())
    else:
        off = act[:, 0] == 0
        assert np.array_equal(R["qd_next"][off], I["qd"][off])


@pytest.mark.parametrize("mu", [0.0, 0.5, 100.0])
@pytest.mark.parametrize("name", CPU_CASES)
def test_warm_start_from_the_converged_impulse_changes_nothing(name, mu):
    I, R = converged(name, mu)
    again = solve(name, I, mu, 5, init=R["impulse"])
    scale = max(1.0, np.abs(R["impulse"]).max())
    assert np.abs(again["impulse"] - R["impulse"]).max() <= 1.0e-13 * scale
    assert again["residual"].max() <= 1.0e-13 * scale


def test_a_bad_normal_or_a_bad_trace_is_nan_in_its_own_configuration_only():
    name = "humanoid30"
    I = make_inputs(name, 8)
    good = solve(name, I, 0.5, 10)
    I["normals"][3, 2] = 0.0
    R = solve(name, I, 0.5, 10)
    assert np.isnan(R["impulse"][3]).all() and np.isnan(R["qd_next"][3]).all() and np.isnan(R["residual"][3])
    keep = np.arange(8) != 3
    assert np.array_equal(R["impulse"][keep], good["impulse"][keep]) and np.array_equal(R["qd_next"][keep], good["qd_next"][keep])
    act = np.ones((8, 4), dtype=np.int32)
    act[3, 2] = 0  # the contact with the bad normal is open: nothing is wrong with the configuration
    R = solve(name, I, 0.5, 10, active=act)
    assert not np.isnan(R["impulse"]).any() and not R["impulse"][3, 2].any()


def test_fp32_rounding_of_the_problem_moves_the_solution_by_rounding(capsys):
    """How far S and b rounded to fp32 move the fp64 iterates: the figure the device's fp32 form is read against."""
    for name in CPU_CASES:
        I = make_inputs(name, B_CPU, dtype=np.float32)
        full, rounded = solve(name, I, 0.5, 200), solve(name, I, 0.5, 200, precision=np.float32)
        moved = np.abs(full["impulse"] - rounded["impulse"]).max()
        print(f"{name}: S and b in fp32 move the impulses by {moved:.2e} (|lam| <= {np.abs(full['impulse']).max():.2f})")
        assert moved <= 1.0e-4
