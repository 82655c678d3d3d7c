"""Pins of the CPU checker of the frictional contact impulses (tests/contact_dynamics_check.py) by facts not of its own making -- the
frictionless solution by enumeration of the pressing sets, the stick solution of the dense KKT checker, the cone and the optimality
residual -- and the case builders the device tests share.  No GPU."""
import zlib

import numpy as np
import pytest

import constrained_dynamics_check as cc
import contact_dynamics_check as cd
import kinematics_check as kc
from helpers import U32, close_aba
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
# every K the two kernel builds (4 and 8 unrolled contacts) take with idle register slots, beside CASES so that the tests parametrised
# over CASES run what they ran; humanoid30_k8_soft: the singular S of humanoid30_k8 with a compliance large enough that the term
# eps lambda_k shows after a few sweeps in fp32 (test_planted_faults_are_rejected)
WIDE_CASES = {
    "humanoid30_k3": ("humanoid30", [6, 12, 19], 0.0),
    "humanoid30_k5": ("humanoid30", [6, 12, 19, 23, 3], 0.0),
    "humanoid30_k6": ("humanoid30", [6, 12, 19, 23, 3, 9], 0.0),
    "humanoid30_k7": ("humanoid30", [6, 12, 19, 23, 3, 9, 15], 0.0),
    "humanoid30_k8_soft": ("humanoid30", [6, 6, 6, 6, 12, 12, 12, 12], 0.05),
}
MIXED_MU = (0.0, 0.3, 0.5, 0.8, 1.2, 2.0, 100.0, 0.6)  # cut to K: frictionless, sliding, sticking, no two neighbours alike
B_CPU = 64
_MODELS = {}


def case_of(name):
    return CASES[name] if name in CASES else WIDE_CASES[name]


def mixed_mu(K):
    return list(MIXED_MU[:K])


def model_of(name):
    key = case_of(name)[0]
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
    _, targets, eps = case_of(name)
    K = len(targets)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 977 * seed)
    q, qd = states(sys_, desc, B, seed=23 + seed)
    poses = corner_poses(K) if K == 8 else kc.random_poses(rng, K)
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


# ---- every K, unequal coefficients, the projection at large mu, and the comparisons of tests/test_gpu_contact_dynamics_wide.py


@pytest.mark.parametrize("name", ["humanoid30_k3", "humanoid30_k5", "humanoid30_k6"])
def test_mixed_mu_converges_with_each_contact_in_its_own_cone(name):
    """MIXED_MU, every contact closed, 1000 sweeps: optimal, every impulse inside the cone of its own coefficient, the mu = 0 contact's
    along its normal, and a sliding contact on its own cone where no neighbour's coefficient would put it.  (humanoid30_k7 reaches a
    natural residual of 1.9e-6 only: no convergence is claimed there, as for humanoid30_k8.)"""
    I = make_inputs(name, B_CPU, seed=1)
    K = len(I["targets"])
    mu = np.array(mixed_mu(K))
    R = solve(name, I, list(mu), 1000)
    lam = lam_of(R)
    scale = max(1.0, np.abs(lam).max())
    nat = cd.natural_residual(R["S"], R["b"], R["n"], mu, None, I["compliance"], lam).max()
    same = lam_of(solve(name, I, 0.5, 1000))
    print(f"{name}: natural residual {nat:.2e}, |lam| <= {scale:.2f}, cond_kkt <= {R['cond_kkt'].max():.2e}, cond_H <= {R['cond_H'].max():.2e}, "
          f"mu = 0.5 everywhere is {np.abs(lam - same).max():.2f} away")
    assert nat <= 1.0e-9 * scale
    ln = np.einsum("bki,bki->bk", R["n"], lam)
    lt = np.linalg.norm(lam - ln[:, :, None] * R["n"], axis=2)
    assert ln.min() >= 0.0 and (lt <= mu * ln * (1.0 + 1.0e-12) + 1.0e-14 * scale).all()  # (forming lt rounds at |lam| u)
    assert lt[:, 0].max() <= 1.0e-14 * scale and ln[:, 0].max() > 0.1  # mu_0 = 0: along the normal, and pressing somewhere
    up = (R["b"] + np.einsum("bij,bj->bi", R["S"], lam.reshape(B_CPU, -1)) + I["compliance"] * lam.reshape(B_CPU, -1)).reshape(B_CPU, K, 3)
    ut = up - np.einsum("bki,bki->bk", R["n"], up)[:, :, None] * R["n"]
    sliding = (np.linalg.norm(ut, axis=2) > 1.0e-6) & (ln > 1.0e-3) & (mu > 0.0)
    assert sliding.any()
    assert np.abs(lt - mu * ln)[sliding].max() <= 1.0e-10 * scale
    off = np.array([[min(abs(lt[r, k] - m * ln[r, k]) for m in mu if m != mu[k]) for k in range(K)] for r in range(B_CPU)])
    assert off[sliding].max() > 1.0e-3  # ... its own: every other coefficient of the list misses by far
    assert np.abs(lam - same).max() > 1.0


def project_plain(x, n, mu):
    """the projection as the header states it, s' = (s + mu r) / (1 + mu^2): mu^2 overflows from 1.34e154 (fp32: 1.85e19)"""
    s = (n * x).sum(axis=1)
    t = x - s[:, None] * n
    r = np.sqrt((t * t).sum(axis=1))
    inside = r <= mu * s
    polar = ~inside & (mu * r <= -s)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s1 = (s + mu * r) / (1.0 + mu * mu)
        y = s1[:, None] * n + (mu * s1 / r)[:, None] * t
    return np.where(inside[:, None], x, np.where(polar[:, None], 0.0, y))


def test_project_at_large_mu_is_the_projection_onto_the_half_space():
    rng = np.random.default_rng(8)
    x = np.concatenate([[[0.3, -0.4, -0.2]], rng.uniform(-1.0, 1.0, (511, 3))])
    n = np.concatenate([[[0.0, 0.0, 1.0]], rng.normal(size=(511, 3))])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    half = x - np.minimum((n * x).sum(axis=1), 0.0)[:, None] * n
    assert ((n * x).sum(axis=1) < 0).sum() > 100
    near = cd.project(x, n, 1.0e10)
    for mu in (1.0e20, 1.0e154, 1.0e200, 1.0e308):
        y = cd.project(x, n, mu)
        assert np.isfinite(y).all() and np.abs(y - half).max() <= 1.0e-15, mu
        assert np.abs(y - near).max() <= 1.0e-9, mu  # continuous in mu: 1e10 is r / mu = 1e-10 away
    assert np.abs(cd.project(x, n, 1.0e20)[0] - [0.3, -0.4, 0.0]).max() <= 1.0e-15
    assert not project_plain(x, n, 1.0e200)[0].any()  # what the stated form gives: the origin
    for mu in (0.0, 0.3, 0.5, 1.0, 1.2, 2.0, 100.0):
        assert np.abs(cd.project(x, n, mu) - project_plain(x, n, mu)).max() <= 1.0e-15, mu
    for mu in (0.0, 0.3, 1.0):  # up to mu = 1 the operations are the stated ones
        assert np.array_equal(cd.project(x, n, mu), project_plain(x, n, mu))


def stale_start(I):
    """an impulse_init no earlier call returned: 5 times the given normal read as a vector of the target frame (outside most cones),
    nonzero angular rows, open contacts included"""
    B, K = I["normals"].shape[:2]
    init = np.empty((B, K, 6))
    init[:, :, 3:] = 5.0 * I["normals"]
    init[:, :, :3] = 0.25 + 0.125 * np.arange(3)
    return init


def held_to_kkt(v, p, R, rows, n_joints, u, label):
    """(qd_out, impulse_out) of configurations `rows` of the checker result R under close_aba with the stick system's cond_inf(KKT)"""
    B = v.shape[0]
    return close_aba(np.concatenate([v, p.reshape(B, -1)], axis=1), np.concatenate([R["qd_next"][rows], R["impulse"][rows].reshape(B, -1)], axis=1), None,
                     n_joints, u, label=label + " (qd+, impulse)", conds=R["cond_kkt"][rows])


def held_to_H(p, R, rows, n_joints, u, label):
    """impulse_out after a few sweeps under close_aba with cond_inf(H): what conditions the formation of S = J H^-1 J^T"""
    B = p.shape[0]
    return close_aba(p.reshape(B, -1), R["impulse"][rows].reshape(B, -1), None, n_joints, u, label=label + " impulse", conds=R["cond_H"][rows])


FAULTS = ("mu0", "normals_raw", "start_unprojected", "start_angular", "untransposed", "no_eps", "v_index")


def solve_with_fault(name, I, mu, iterations, fault, active=None, v_normal=None, init=None, T=None):
    """dict(qd_next, impulse, residual): the checker's terms, sweeps and velocity update with ONE planted fault -- what a kernel wrong in that one
    place returns.  fault=None is cd.contact_impulse to the bit.  T: cd.terms of these inputs and v_normal, where the caller has them."""
    assert fault is None or fault in FAULTS
    _, desc, om = model_of(name)
    B, K = I["qd"].shape[0], len(I["targets"])
    mu = np.asarray(mu, dtype=float)
    T = T or cd.terms(om, desc, I["q"], I["qd"], I["targets"], I["poses"], I["normals"], v_normal)
    S, b, n, eps = T["S"].copy(), T["b"], T["n"], I["compliance"]
    act = cd._active(active, B, K)
    v = np.zeros((B, K)) if v_normal is None else np.asarray(v_normal, dtype=float)
    lam = np.zeros((B, K, 3))
    if fault == "mu0":  # contact 0's coefficient for every contact
        mu = np.full(K, mu[0])
    if fault == "normals_raw":  # the given normals as they are
        n = n * T["norm"][:, :, None]
    if fault == "v_index":  # v_normal of the neighbouring contact
        v = np.roll(v, 1, axis=1)
    if fault in ("normals_raw", "v_index"):
        b = np.einsum("bij,bj->bi", T["Jl"], I["qd"]) - (v[:, :, None] * n).reshape(B, -1)
    if fault == "untransposed":  # block (k, l), l > k, read as block (l, k) without the transpose, in the second half of the unrolled contacts
        for k in range(4, K):
            for l in range(k + 1, K):
                S[:, 3 * k:3 * k + 3, 3 * l:3 * l + 3] = S[:, 3 * l:3 * l + 3, 3 * k:3 * k + 3]
    if init is not None:
        x0 = np.asarray(init, dtype=float).reshape(B, K, 6)
        x0 = x0[:, :, 3:] + (x0[:, :, :3] if fault == "start_angular" else 0.0)
        for k in range(K):
            lam[:, k] = np.where(act[:, k, None], x0[:, k] if fault == "start_unprojected" else cd.project(x0[:, k], n[:, k], mu[k]), 0.0)
    res = np.zeros(B)
    for _ in range(iterations):
        res = np.zeros(B)
        for k in range(K):
            rows = slice(3 * k, 3 * k + 3)
            u = b[:, rows] + np.einsum("bij,bj->bi", S[:, rows, :], lam.reshape(B, -1)) + (0.0 if fault == "no_eps" else eps) * lam[:, k]
            rho = 1.0 / (S[:, 3 * k, 3 * k] + S[:, 3 * k + 1, 3 * k + 1] + S[:, 3 * k + 2, 3 * k + 2] + eps)
            new = np.where(act[:, k, None], cd.project(lam[:, k] - rho[:, None] * u, n[:, k], mu[k]), 0.0)
            res = np.maximum(res, np.abs(new - lam[:, k]).max(axis=1))
            lam[:, k] = new
    impulse = np.zeros((B, K, 6))
    impulse[:, :, 3:] = lam
    qd_next = I["qd"] + np.linalg.solve(T["H"], np.einsum("bji,bj->bi", T["Jl"], lam.reshape(B, -1))[:, :, None])[:, :, 0]
    return dict(qd_next=qd_next, impulse=impulse, residual=res)


ACTIVE_VALUES = np.array([1, -1, 7], dtype=np.int32)  # "nonzero = closed": not 1 alone
FEW_SWEEPS_CASES = ["humanoid30_k8", "humanoid30_k7", "humanoid30", "humanoid30_k8_soft"]
MANY_SWEEPS = {"humanoid30_k3": 50, "humanoid30_k5": 50, "humanoid30_k6": 50, "humanoid30_k7": 20}  # k7: no convergence is claimed


def wide_inputs(name, B, dtype=np.float64, seed=1):
    """make_inputs with the closed contacts marked by 1, -1 or 7"""
    I = make_inputs(name, B, seed=seed, dtype=dtype)
    I["active"] = I["active"] * np.random.default_rng(B + seed).choice(ACTIVE_VALUES, size=I["active"].shape)
    return I


def test_planted_faults_are_rejected_by_the_comparisons_of_the_device_tests():
    """Each fault of FAULTS planted into the checker's sweeps, held to the comparison the device test calls on the inputs it calls it
    on, in the weaker precision (fp32-rounded inputs, u = 2^-24): close_aba must raise.  few sweeps from a stale start: impulse_out under
    cond_inf(H) (held_to_H); many sweeps from zero: (qd_out, impulse_out) under cond_inf(KKT) (held_to_kkt); the normals' scaling: bits.
    The same sweeps on S and b rounded to fp32 -- what the precision itself does -- stay inside both."""
    B, rows = 65, slice(0, 65)
    rejected = set()
    for name in FEW_SWEEPS_CASES + list(MANY_SWEEPS):
        I = wide_inputs(name, B, np.float32)
        _, desc, om = model_of(name)
        K, n = len(I["targets"]), desc.n_joints
        mu = mixed_mu(K)
        T = cd.terms(om, desc, I["q"], I["qd"], I["targets"], I["poses"], I["normals"], I["v_normal"])
        plans = ([("H", s, stale_start(I)) for s in (1, 3)] if name in FEW_SWEEPS_CASES else []) + \
                ([("kkt", MANY_SWEEPS[name], None)] if name in MANY_SWEEPS else [])
        for kind, sweeps, init in plans:
            R = solve(name, I, mu, sweeps, active=I["active"], v_normal=I["v_normal"], init=init)
            hold = (lambda G, label: held_to_H(G["impulse"], R, rows, n, U32, label)) if kind == "H" else \
                   (lambda G, label: held_to_kkt(G["qd_next"], G["impulse"], R, rows, n, U32, label))
            same = solve_with_fault(name, I, mu, sweeps, None, I["active"], I["v_normal"], init, T)
            assert all(np.array_equal(same[k], R[k]) for k in ("impulse", "qd_next", "residual"))
            hold(solve(name, I, mu, sweeps, active=I["active"], v_normal=I["v_normal"], init=init, precision=np.float32), f"{name} {sweeps} sweeps, S and b in fp32")
            faults = ["mu0", "v_index"] + (["start_unprojected", "start_angular"] if init is not None else []) + (["untransposed"] if K >= 6 else []) + \
                     (["no_eps"] if name == "humanoid30_k8_soft" and kind == "H" else [])
            for fault in faults:
                G = solve_with_fault(name, I, mu, sweeps, fault, I["active"], I["v_normal"], init, T)
                with pytest.raises(AssertionError, match="worst row"):
                    hold(G, f"planted {fault}: {name} {sweeps} sweeps")
                rejected.add(fault)
    # the normals: the device test scales each by a power of two and asks for the bits of the unscaled call
    name = "humanoid30_k5"
    I = wide_inputs(name, B, np.float32)
    mu = mixed_mu(5)
    R = solve(name, I, mu, 30, active=I["active"], v_normal=I["v_normal"])
    scaled = dict(I, normals=I["normals"] * 2.0 ** np.random.default_rng(6).integers(-10, 11, (B, 5, 1)))
    again = solve(name, scaled, mu, 30, active=I["active"], v_normal=I["v_normal"])
    assert np.array_equal(again["impulse"], R["impulse"]) and np.array_equal(again["qd_next"], R["qd_next"]) and np.array_equal(again["residual"], R["residual"])
    with np.errstate(all="ignore"):  # (normals of length 1024 make the sweeps diverge)
        G = solve_with_fault(name, scaled, mu, 30, "normals_raw", I["active"], I["v_normal"])
    assert not np.array_equal(G["impulse"], R["impulse"]) and not np.array_equal(G["qd_next"], R["qd_next"])
    rejected.add("normals_raw")
    assert rejected == set(FAULTS)
