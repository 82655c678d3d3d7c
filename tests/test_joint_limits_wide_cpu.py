"""The case builders of tests/test_gpu_joint_limits_wide.py and their pins: the wide comb at the cap of the list length, designed closure
patterns, one range per row, permuted lists, infinite and degenerate ranges, warm starts -- and the mistakes a kernel could make on exactly
those inputs, each held to the comparison the device tests make (close_aba on (qd+, impulse) with the stick system's cond_inf at the fp32
unit roundoff).  No GPU."""
import numpy as np
import pytest

import joint_limits_check as jl
from helpers import U32, close_aba, f32_aba_forward_factor
from test_joint_limits_cpu import COMB_CHAINS, COMB_DEPTH, ERP, LOWER, MARGIN, UPPER, make_inputs, model_of, solve
from test_kinematics_cpu import states

B_WIDE = 65    # one full wave and a ragged one of one lane
B_SPARSE = 130  # two full waves and a ragged one of two lanes
INF = np.inf


def comb_order():
    """comb16x4 interleaved by depth: joint 0 of every chain, then joint 1 of every chain, ... -- coupled rows are 16 apart in the list"""
    return [COMB_DEPTH * c + k for k in range(COMB_DEPTH) for c in range(COMB_CHAINS)]


def row_ranges(L):
    """one range per row, distinct, asymmetric, exact in fp32: [-1 - i / 16, 0.5 + i / 32]"""
    i = np.arange(L)
    return -1.0 - i / 16.0, 0.5 + i / 32.0


def mixed_ranges(L):
    """rows i = 0, 1, 2, 3, 4 (mod 5): no lower limit, no upper limit, neither, lower == upper, a finite range.  The finite limits,
    [-0.5 - i / 32, 0.25 + i / 64], are inside what a prismatic joint's state reaches, at margin 0 too."""
    i = np.arange(L)
    lower, upper = -0.5 - i / 32.0, 0.25 + i / 64.0
    lower, upper = np.where((i % 5 == 0) | (i % 5 == 2), -INF, lower), np.where((i % 5 == 1) | (i % 5 == 2), INF, upper)
    pinned = i % 5 == 3
    return np.where(pinned, 0.25 * (i % 3 - 1.0), lower), np.where(pinned, 0.25 * (i % 3 - 1.0), upper)


def wide_inputs(name, B, seed=0, dtype=np.float64, joints=None, lower=None, upper=None, margins=(MARGIN,), erp=ERP):
    """make_inputs with the list in the order given and one range per row.  A q of a listed joint within 1e-3 of one of its row's own
    thresholds -- lower_i + margin, upper_i - margin for every margin the case is run with, and the middle of a range too narrow for an
    open row, where the side changes -- is moved 2e-3 away from it.  dict(..., margin=margins[0])."""
    sys_, desc, om = model_of(name)
    joints = (comb_order() if name == "comb16x4" else jl.one_dof_joints(desc)) if joints is None else list(joints)
    L = len(joints)
    lower = np.full(L, LOWER) if lower is None else np.asarray(lower, dtype=float)
    upper = np.full(L, UPPER) if upper is None else np.asarray(upper, dtype=float)
    q, qd = states(sys_, desc, B, seed=31 + seed)
    _, c = jl.joint_indices(desc, joints)
    for i in range(L):
        marks = [lower[i] + m for m in margins] + [upper[i] - m for m in margins]
        if upper[i] - lower[i] <= 2.0 * max(margins):
            marks.append(0.5 * (lower[i] + upper[i]))
        for t in marks:
            if np.isfinite(t):
                x = q[:, c[i]]
                q[:, c[i]] = np.where(np.abs(x - t) < 1.0e-3, t + np.where(x >= t, 2.0e-3, -2.0e-3), x)
    r = lambda x: np.asarray(x).astype(dtype).astype(np.float64)
    return dict(q=r(q), qd=r(qd), joints=joints, lower=lower, upper=upper, margin=margins[0], erp=erp)


def shuffled(joints, seed=5):
    return [int(j) for j in np.random.default_rng(seed).permutation(joints)]


def start_of(I, dtype=np.float64, seed=17):
    """a warm start that has nothing to do with the solution: twice a standard-normal draw, nonzero on every row, open ones too"""
    B, L = I["q"].shape[0], len(I["joints"])
    return (2.0 * np.random.default_rng(seed).normal(size=(B, L))).astype(dtype).astype(np.float64)


# (configuration, row) -> q of that row's joint.  Range +-1, margin 0.25: -1.125 / 1.25 are violated, -0.875 / 0.8125 merely near.
# Wave 0: rows closed in lanes 5, 40 and 63 only -- row 2 in exactly one lane, row 7 in two lanes on opposite sides, lane 40 with many rows
# beside lanes with none.  Wave 1: row 9 in lane 0 alone.  The ragged wave (configurations 128, 129): nothing.
SPARSE_PATTERN = {(5, 2): -1.125, (5, 7): 0.8125, (5, 11): -0.875,
                  (40, 0): 1.25, (40, 3): -1.125, (40, 7): -1.125, (40, 8): 0.8125, (40, 12): 1.25, (40, 15): -0.875, (40, 16): 1.25, (40, 20): -1.125,
                  (40, 23): 0.8125,
                  (63, 11): 1.25, (63, 23): -1.125,
                  (64, 9): -1.125}


def designed_inputs(name, B, pattern, seed=0, dtype=np.float64):
    """make_inputs with every listed q clipped into [-0.5, 0.5] -- nothing closed -- and then the chosen (configuration, row) pairs put
    where the pattern says"""
    I = make_inputs(name, B, seed, dtype)
    _, desc, om = model_of(name)
    _, c = jl.joint_indices(desc, I["joints"])
    q = I["q"].copy()
    q[:, c] = np.clip(q[:, c], -0.5, 0.5)
    for (cfg, row), value in pattern.items():
        q[cfg, c[row]] = value
    return dict(I, q=q.astype(dtype).astype(np.float64))


def designed_closure(B, L, pattern):
    closed = np.zeros((B, L), dtype=bool)
    for cfg, row in pattern:
        closed[cfg, row] = True
    return closed


# ---- the cases of the device tests: name -> (model, inputs of B configurations rounded to dtype)
def humanoid_joints(L):
    return jl.one_dof_joints(model_of("humanoid30")[1])[:L]


def wide_case(case, dtype=np.float64):
    kind, _, what = case.partition(":")
    if kind == "warm":  # the range +-1 on every row and a start that is far off.  erp 1: at the 50 of make_inputs the impulses reach 2e3, and
        # what a start of size 2 changes is lost in the fp32 bound of the humanoid, whose cond_kkt is 1e4
        I = wide_inputs(what, B_WIDE, seed=7, dtype=dtype, erp=1.0)
        return what, dict(I, init=start_of(I, dtype))
    if kind == "order":  # one range per row, the list out of joint order
        name, joints = {"humanoid30_l24_shuffled": ("humanoid30", shuffled(humanoid_joints(24))),
                        "humanoid30_l24_reversed": ("humanoid30", humanoid_joints(24)[::-1]),
                        "humanoid30_l22_shuffled": ("humanoid30", shuffled(humanoid_joints(22), seed=6)),
                        "onedof12": ("onedof12", shuffled(jl.one_dof_joints(model_of("onedof12")[1]), seed=7)),
                        "mixed12": ("mixed12", shuffled(jl.one_dof_joints(model_of("mixed12")[1]), seed=8))}[what]
        lower, upper = row_ranges(len(joints))
        return name, wide_inputs(name, B_WIDE, seed=8, dtype=dtype, joints=joints, lower=lower, upper=upper)
    if kind == "sparse":  # with a -0.0 in the velocities of a configuration that has no closed row: its qd_out is held to the bits of qd
        I = designed_inputs("humanoid30", B_SPARSE, SPARSE_PATTERN if what == "designed" else {}, seed=9, dtype=dtype)
        I["qd"][41, 3] = -0.0
        return "humanoid30", I
    if kind == "inf":  # run with margin 0.25 and 0, erp 50 and 0
        L = len(jl.one_dof_joints(model_of(what)[1]))
        lower, upper = mixed_ranges(L)
        return what, wide_inputs(what, B_WIDE, seed=10, dtype=dtype, lower=lower, upper=upper, margins=(MARGIN, 0.0))
    if kind == "comb":  # the first L entries of the interleaved list
        return "comb16x4", wide_inputs("comb16x4", B_WIDE, seed=1, dtype=dtype, joints=comb_order()[:int(what)])
    raise KeyError(case)


_SOLVED = {}


def solved(case, dtype=np.float64, sweeps=3, compliance=0.0, **over):
    """(model name, inputs, checker result), once per key; the start of the inputs, where they have one, is used"""
    key = (case, np.dtype(dtype).name, sweeps, compliance, tuple(sorted(over.items())))
    if key not in _SOLVED:
        name, I = wide_case(case, dtype)
        I = dict(I, **over)
        _SOLVED[key] = (name, I, solve(name, I, sweeps, compliance, I.get("init")))
    return _SOLVED[key]


def prismatic_rows(name, I):
    _, desc, om = model_of(name)
    return np.array([int(desc.joint_type[j]) == 1 for j in I["joints"]])


# ---- (a) the comb
def test_the_comb_is_wide_and_well_conditioned():
    """64 one-DoF joints in 16 chains of 4 on a fixed root, 12 of them prismatic; in the interleaved list the rows of a chain are 16
    apart.  With fp32-rounded states the fp32 bound of the device test, 8 sqrt(8 n) cond_kkt 2^-24, is <= 5e-2 on every configuration
    and <= 1e-2 at the median: it says something about every number (on tree128 it is of order 1e2)."""
    _, desc, om = model_of("comb16x4")
    assert desc.n_joints == 64 and desc.nv == 64 and desc.nq == 64
    assert [int(p) for p in desc.parent] == [-1 if j % COMB_DEPTH == 0 else j - 1 for j in range(64)]
    assert [int(t) for t in desc.joint_type] == [1 if j % 5 == 4 else 0 for j in range(64)]
    order = comb_order()
    assert sorted(order) == list(range(64)) and order[:3] == [0, 4, 8] and all(order[i + 16] == order[i] + 1 for i in range(48))
    name, I, R = solved("comb:64", np.float32, sweeps=3)
    assert I["joints"] == order and not R["bad"].any()
    bound = f32_aba_forward_factor(desc.n_joints) * R["cond_kkt"] * U32
    share = R["closed"].mean()
    print(f"comb16x4: cond_kkt median {np.median(R['cond_kkt']):.2e} max {R['cond_kkt'].max():.2e}, fp32 bound median {np.median(bound):.2e} max {bound.max():.2e}, "
          f"{100 * share:.0f} % closed")
    assert bound.max() <= 5.0e-2 and np.median(bound) <= 1.0e-2
    assert (R["s"][R["closed"]] > 0).any() and (R["s"][R["closed"]] < 0).any() and 0.5 <= share <= 0.8
    assert R["closed"][:, prismatic_rows(name, I)].any() and np.abs(R["impulse"]).max() > 0.1
    for L in (32, 33):  # the shorter lists are no worse
        _, _, RL = solved(f"comb:{L}", np.float32, sweeps=3)
        assert not RL["bad"].any() and (f32_aba_forward_factor(desc.n_joints) * RL["cond_kkt"] * U32).max() <= 5.0e-2


# ---- (b) designed closure
def test_the_designed_closure_is_exactly_the_designed_one():
    name, I, R = solved("sparse:designed")
    L = len(I["joints"])
    want = designed_closure(B_SPARSE, L, SPARSE_PATTERN)
    assert np.array_equal(R["closed"], want) and not R["bad"].any()
    per_lane = want[:64].sum(axis=0)
    assert sorted(set(np.nonzero(want[:64].any(axis=1))[0])) == [5, 40, 63] and per_lane[2] == 1 and per_lane[7] == 2
    assert R["s"][5, 7] == -R["s"][40, 7] and want[40].sum() >= 8 and not want[39].any() and not want[41].any()
    assert np.nonzero(want[64:128])[0].tolist() == [0] and not want[128:].any()
    assert (R["gap"][want] < 0).any() and (R["gap"][want] > 0).any() and (R["s"][want] > 0).any() and (R["s"][want] < 0).any()
    violated = want & (R["gap"] < 0)
    assert (np.abs(R["impulse"][violated]) > 0.1).all() and np.abs(R["impulse"]).max() > 5.0, np.abs(R["impulse"]).max()
    idle = ~want.any(axis=1)
    assert idle[41] and I["qd"][41, 3] == 0 and np.signbit(I["qd"][41, 3])
    assert idle.sum() == B_SPARSE - 4 and np.array_equal(R["qd_next"][idle], I["qd"][idle]) and not R["impulse"][idle].any() and not R["residual"][idle].any()
    assert (R["qd_next"][~idle] != I["qd"][~idle]).any(axis=1).all()
    _, I0, R0 = solved("sparse:none")
    assert not R0["closed"].any() and np.array_equal(R0["qd_next"], I0["qd"]) and not R0["bad"].any()


# ---- (c) ranges and lists
def test_ranges_and_lists_are_what_they_claim():
    lower, upper = row_ranges(64)
    for x in (lower, upper, *mixed_ranges(64)):
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    assert len(set(lower)) == 64 and len(set(upper)) == 64 and (lower != -upper).all() and (lower < upper).all()
    lo, hi = mixed_ranges(8)
    kinds = [(np.isneginf(a), np.isposinf(b), a == b) for a, b in zip(lo, hi)]
    assert kinds[:5] == [(True, False, False), (False, True, False), (True, True, False), (False, False, True), (False, False, False)]
    for case in ("order:humanoid30_l24_shuffled", "order:humanoid30_l24_reversed", "order:humanoid30_l22_shuffled", "order:onedof12", "order:mixed12"):
        name, I = wide_case(case)
        _, desc, om = model_of(name)
        every = jl.one_dof_joints(desc)[:len(I["joints"])]
        assert sorted(I["joints"]) == every and I["joints"] != every
        assert sum(a > b for a, b in zip(I["joints"][1:], I["joints"][:-1])) < len(every) - 1  # not ascending
    assert wide_case("order:humanoid30_l24_reversed")[1]["joints"] == humanoid_joints(24)[::-1]
    for case, margins in (("order:mixed12", (MARGIN,)), ("inf:humanoid30", (MARGIN, 0.0)), ("inf:mixed12", (MARGIN, 0.0)), ("comb:64", (MARGIN,))):
        for dtype in (np.float64, np.float32):
            name, I = wide_case(case, dtype)
            _, c = jl.joint_indices(model_of(name)[1], I["joints"])
            for m in margins:
                for t in (I["lower"] + m, I["upper"] - m):
                    ok = np.isfinite(t)
                    assert np.abs(I["q"][:, c][:, ok] - t[ok]).min() >= 1.0e-3 - 1.0e-6
            pinned = I["lower"] == I["upper"]
            if pinned.any():
                assert np.abs(I["q"][:, c][:, pinned] - I["lower"][pinned]).min() >= 1.0e-3 - 1.0e-6


@pytest.mark.parametrize("case", ["order:humanoid30_l24_shuffled", "order:humanoid30_l24_reversed", "order:onedof12", "order:mixed12"])
def test_the_order_of_the_list_shows_early_and_not_in_the_solution(case):
    """The complementarity problem has one solution whatever the order of its rows: 1000 sweeps over the list in joint order, its ranges
    carried along, end where 1000 sweeps over the permuted list end, row for row.  After 3 sweeps the two differ."""
    name, I, R3 = solved(case, sweeps=3)
    _, desc, om = model_of(name)
    order = np.argsort(I["joints"])
    J = dict(I, joints=[I["joints"][k] for k in order], lower=I["lower"][order], upper=I["upper"][order])
    assert J["joints"] == sorted(I["joints"])
    A3 = solve(name, J, 3)
    assert np.array_equal(A3["closed"], R3["closed"][:, order]) and not R3["bad"].any()
    assert np.abs(A3["impulse"] - R3["impulse"][:, order]).max() > 0.1
    P, A = solve(name, I, 1000), solve(name, J, 1000)
    scale = max(1.0, np.abs(A["impulse"]).max())
    assert np.abs(A["impulse"] - P["impulse"][:, order]).max() <= 1.0e-8 * scale and np.abs(A["qd_next"] - P["qd_next"]).max() <= 1.0e-8 * scale
    if name != "humanoid30":
        pressing = (np.abs(R3["impulse"]) > 0.1) & prismatic_rows(name, I)[None, :]
        assert pressing.any()  # a prismatic row is closed and presses
        assert not np.array_equal(R3["d"], R3["c"])


@pytest.mark.parametrize("name", ["humanoid30", "mixed12"])
def test_infinite_and_degenerate_ranges_in_the_checker(name):
    """A limit at infinity never closes, a row with neither limit holds exactly 0 and the rows with lower == upper are always closed; no
    configuration is bad, at erp 0 (where erp gap is 0 inf) and margin 0 too.  The rows with one limit are those of the same range with
    the other limit far away."""
    for margin, erp in ((MARGIN, ERP), (0.0, 0.0), (0.0, ERP), (MARGIN, 0.0)):
        _, I, R = solved("inf:" + name, sweeps=3, margin=margin, erp=erp)
        lo, hi = I["lower"], I["upper"]
        assert not R["bad"].any() and np.isfinite(R["qd_next"]).all() and np.isfinite(R["impulse"]).all()
        both, pinned = np.isinf(lo) & np.isinf(hi), lo == hi
        assert both.any() and pinned.any() and not R["closed"][:, both].any() and not R["impulse"][:, both].any() and R["closed"][:, pinned].all()
        assert not (R["closed"] & (R["s"] > 0))[:, np.isinf(lo)].any() and not (R["closed"] & (R["s"] < 0))[:, np.isinf(hi)].any()
        assert R["closed"][:, np.isinf(lo) & ~both].any() and R["closed"][:, np.isinf(hi) & ~both].any()
        far = solve(name, dict(I, lower=np.where(np.isinf(lo), -1.0e6, lo), upper=np.where(np.isinf(hi), 1.0e6, hi)), 3)
        assert np.array_equal(far["closed"], R["closed"]) and np.array_equal(far["impulse"], R["impulse"]) and np.array_equal(far["qd_next"], R["qd_next"])
    assert np.abs(R["impulse"]).max() > 0.1


# ---- (d) planted faults
def sweep_from(S, b, closed, eps, iterations, lam):
    """joint_limits_check.sweeps from a start taken as it is"""
    lam = lam.copy()
    for _ in range(iterations):
        for i in range(b.shape[1]):
            u = b[:, i] + np.einsum("bj,bj->b", S[:, i, :], lam) + eps * lam[:, i]
            lam[:, i] = np.where(closed[:, i], np.maximum(0.0, lam[:, i] - u / (S[:, i, i] + eps)), 0.0)
    return lam


def planted(name, I, fault, iterations, compliance=0.0):
    """(qd_next, impulse) of the checker's sweeps with one mistake a kernel could make; fault None: the checker itself"""
    _, desc, om = model_of(name)
    L = len(I["joints"])
    order = np.argsort(I["joints"])  # list positions in joint order
    lower, upper = I["lower"], I["upper"]
    if fault == "ranges in joint order":  # row i takes the range given for the i-th of the listed joints in joint order
        lower, upper = lower[order], upper[order]
    T = jl.terms(om, desc, I["q"], I["qd"], I["joints"], lower, upper, I["margin"], I["erp"])
    s, closed, d, S, b = T["s"], T["closed"], T["d"], T["S"], T["b"]
    full = T["Hinv"][:, d][:, :, d]
    if fault == "triangle transposed":  # j < i: row d_j of column i
        block = np.triu(full) + np.triu(full, 1).transpose(0, 2, 1)
        S = s[:, :, None] * block * s[:, None, :]
    elif fault == "row at the list position":  # j < i: row i, not row d_i, of column j
        low = np.tril(T["Hinv"][:, :L][:, :, d])
        S = s[:, :, None] * (low + np.tril(low, -1).transpose(0, 2, 1)) * s[:, None, :]
    elif fault == "velocity at the q index":
        b = s * I["qd"][:, np.minimum(T["c"], desc.nv - 1)] + I["erp"] * T["gap"]
    elif fault == "a row closed in one lane dropped":
        for first in range(0, closed.shape[0], 64):
            closed[first:first + 64] &= closed[first:first + 64].sum(axis=0, keepdims=True) >= 2
    init = I.get("init")
    lam0 = np.zeros_like(b) if init is None else s * init
    start = np.where(closed, lam0 if fault == "start not clamped" else np.maximum(0.0, lam0), 0.0)
    b = np.where(closed, b, 0.0)
    if fault == "sweeps in joint order":
        lam = sweep_from(S[:, order][:, :, order], b[:, order], closed[:, order], compliance, iterations, start[:, order])[:, np.argsort(order)]
    else:
        lam = sweep_from(S, b, closed, compliance, iterations, start)
    if fault == "open rows kept":  # the start survives on an open row and is summed
        lam = np.where(closed, lam, np.maximum(0.0, lam0))
        impulse = s * lam
    else:
        impulse = np.where(closed, s * lam, 0.0)
    qd_next = I["qd"].copy()
    for i in range(L):
        qd_next += impulse[:, i, None] * T["Hinv"][:, :, d[i]]
    if fault == "impulses in joint order":
        impulse = impulse[:, order]
    return qd_next, impulse


def compared(name, R, v, p):
    """the device test's comparison of (qd+, impulse) at the fp32 unit roundoff: the achieved share of the bound, or None where it is refused"""
    n = model_of(name)[1].n_joints
    try:
        return close_aba(np.concatenate([v, p], axis=1), np.concatenate([R["qd_next"], R["impulse"]], axis=1), None, n, U32, label=None, conds=R["cond_kkt"])
    except AssertionError:
        return None


WARM_FAULTS = [("warm:humanoid30", "start not clamped"), ("warm:arm7", "start not clamped"), ("warm:comb16x4", "start not clamped"),
               ("warm:humanoid30", "open rows kept"), ("warm:arm7", "open rows kept"), ("warm:comb16x4", "open rows kept")]
FAULTS = [("order:humanoid30_l24_shuffled", "row at the list position"), ("order:humanoid30_l24_shuffled", "sweeps in joint order"),
          ("order:humanoid30_l24_reversed", "sweeps in joint order"), ("order:humanoid30_l22_shuffled", "sweeps in joint order"),
          ("order:humanoid30_l24_shuffled", "ranges in joint order"), ("order:humanoid30_l24_reversed", "ranges in joint order"),
          ("order:humanoid30_l24_shuffled", "impulses in joint order"), ("order:onedof12", "impulses in joint order"),
          ("order:onedof12", "ranges in joint order"), ("order:mixed12", "ranges in joint order"), ("order:mixed12", "velocity at the q index"),
          ("sparse:designed", "a row closed in one lane dropped")]


@pytest.mark.parametrize("case,fault,sweeps", [(c, f, 1) for c, f in WARM_FAULTS] + [(c, f, 3) for c, f in FAULTS])
def test_planted_faults_are_rejected_on_the_inputs_of_the_device_tests(case, fault, sweeps):
    """With sweeps the device tests run -- the first, where a start shows most (after three, what is left of an unclamped start on the
    humanoid is inside the fp32 bound), and three for the rest -- the comparison passes the checker's sweeps restated here (they are the
    checker's, to the bit) and refuses the mistake."""
    name, I, R = solved(case, sweeps=sweeps)
    v, p = planted(name, I, None, sweeps)
    assert np.array_equal(v, R["qd_next"]) and np.array_equal(p, R["impulse"])
    assert compared(name, R, v, p) == 0.0
    assert compared(name, R, *planted(name, I, fault, sweeps)) is None, f"{case}: '{fault}' passes the comparison"


@pytest.mark.parametrize("case", ["order:humanoid30_l24_shuffled", "order:humanoid30_l24_reversed", "order:mixed12"])
def test_the_transposed_triangle_is_the_same_matrix(case):
    """Reading entry (i, j), j < i, as row d_j of column i in place of row d_i of column j is no mistake in any order of the list: the
    inverse of H is symmetric, the two reads differ by what rounding left of that, and no comparison at cond u can or should tell them
    apart -- the device tests' own comparison at the fp64 unit roundoff, the sharpest they make, passes it.  What a list out of joint
    order does show is the order of the sweeps and a row read at the list position, both refused above."""
    name, I, R = solved(case, sweeps=3)
    v, p = planted(name, I, "triangle transposed", 3)
    n = model_of(name)[1].n_joints
    share = close_aba(np.concatenate([v, p], axis=1), np.concatenate([R["qd_next"], R["impulse"]], axis=1), None, n, 2.0 ** -53, label=None,
                      conds=R["cond_kkt"]) / f32_aba_forward_factor(n)
    print(f"{case}: the transposed triangle is at {share:.2e} of the fp64 bound")
