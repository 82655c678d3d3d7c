"""Pins of the CPU checker of the parameter gradients (tests/parameters_vjp_check.py) by central differences of the oracle's own inverse
and forward dynamics (inertial_parameters_check.Checker) over single entries of pi.  No GPU, nothing from the code under test.

The inverse dynamics is linear in (m, m c, J), hence linear -- at most -- in every single one of the ten numbers of a body with the
others held: the central difference is exact up to rounding, |tau| eps / h.  With h = 1e-3, measured: arm7 6.2e-12 at |g| = 9.8, lumped
2.6e-12 at 17, humanoid30 3.6e-11 at |g| = 39; held to 1e-9 max(1, |g|_inf).  The forward dynamics is not linear: with h = 1e-5 the difference
carries a truncation of the order h^2 |d^3 qdd / d pi^3| and a rounding of cond(H) eps |qdd| / h; the first four bodies gave, with and without wrenches, at most arm7 7.9e-10,
lumped 1.8e-8 (at |g| = 34), humanoid30 5.2e-10 (cond_inf(H) 1 030); held to 1e-6 max(1, |g|_inf)."""
import numpy as np
import pytest

import inertial_parameters_check as ipc
import parameters_vjp_check as pc
from test_inertial_parameters_cpu import GRAVITY, batch, make_case

CASES = ["arm7", "lumped", "humanoid30"]
ROWS = 3


def cotangent(B, nv, seed=8):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, nv))


def central_difference(fn, pi, weights, bodies, h):
    """d (weights . fn(pi)) / d pi[r, i, k] for every row r, the bodies i given and k < 10: the entry moves in all rows at once (the rows
    do not see each other)."""
    g = np.zeros((pi.shape[0], len(bodies), 10))
    for a, i in enumerate(bodies):
        for k in range(10):
            up, down = pi.copy(), pi.copy()
            up[:, i, k] += h
            down[:, i, k] -= h
            g[:, a, k] = (weights * (fn(up) - fn(down))).sum(axis=1) / (2.0 * h)
    return g


@pytest.mark.parametrize("case", CASES)
def test_inverse_form_against_central_differences(case):
    sys_, desc = make_case(case)
    q, qd, qdd, _, pi = batch(sys_, desc, ROWS)
    u = cotangent(ROWS, desc.nv)
    g, scale, chi = pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, GRAVITY)
    assert g.shape == (ROWS, desc.n_joints, 10) and (scale > 0.0).all() and (chi >= 1.0).all()
    ck = ipc.Checker(desc)
    fd = central_difference(lambda p: ck.rnea(q, qd, qdd, p, GRAVITY), pi, u, range(desc.n_joints), 1e-3)
    err, bound = np.abs(g - fd).max(), 1e-9 * max(1.0, np.abs(g).max())
    print(f"{case}: |g - fd|_inf = {err:.3e} at |g|_inf = {np.abs(g).max():.3g} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("case", CASES)
def test_inverse_form_switches_are_zero_inputs(case):
    sys_, desc = make_case(case)
    q, qd, qdd, _, pi = batch(sys_, desc, ROWS)
    u = cotangent(ROWS, desc.nv)
    z = np.zeros_like(qd)
    for cc, ca in ((False, True), (True, False), (False, False)):
        got = pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, GRAVITY, cc, ca)[0]
        assert np.array_equal(got, pc.rnea_parameters_vjp(desc, q, qd if cc else z, qdd if ca else z, pi, u, GRAVITY)[0])
    assert not pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, np.zeros_like(u), GRAVITY)[0].any()  # u = 0: zeros


@pytest.mark.parametrize("case", CASES)
def test_forward_form_against_central_differences(case):
    sys_, desc = make_case(case)
    q, qd, _, tau, pi = batch(sys_, desc, ROWS)
    w = cotangent(ROWS, desc.nv, 9)
    f = np.random.default_rng(9).uniform(-5.0, 5.0, (ROWS, desc.n_joints, 6))
    ck = ipc.Checker(desc)
    bodies = range(min(4, desc.n_joints))
    for wrenches in (None, f):
        qdd, mu, g, scale, chi, conds = pc.aba_parameters_vjp(desc, q, qd, tau, pi, w, GRAVITY, wrenches)
        assert np.array_equal(qdd, ck.aba(q, qd, tau, pi, GRAVITY, wrenches))
        H = ck.crba(q, pi)
        assert np.abs(np.einsum("bij,bj->bi", H, mu) - w).max() <= 1e-12 * conds.max()
        fd = central_difference(lambda p: ck.aba(q, qd, tau, p, GRAVITY, wrenches), pi, w, bodies, 1e-5)
        err, bound = np.abs(g[:, :len(bodies)] - fd).max(), 1e-6 * max(1.0, np.abs(g).max())
        print(f"{case}: |g - fd|_inf = {err:.3e} at |g|_inf = {np.abs(g).max():.3g}, cond_inf(H) <= {conds.max():.3g} (bound {bound:.3e})")
        assert err <= bound


def test_chain_rule_and_amplification():
    """g_m = g^_m + c . g^_h, g_c = m g^_h, g_J = g^_J; chi = max(1, m, 1 + |c|_1) over the bodies."""
    pi = np.array([[[2.0, 0.1, -0.2, 0.3, 1, 2, 3, 4, 5, 6], [0.5, 0.0, 0.0, 0.0, 1, 0, 0, 1, 0, 1]]])
    ghat = np.arange(20.0).reshape(1, 2, 10) + 1.0
    g = pc.chain(pi, ghat)
    assert g[0, 0, 0] == ghat[0, 0, 0] + 0.1 * 2.0 - 0.2 * 3.0 + 0.3 * 4.0
    assert np.array_equal(g[0, 0, 1:4], 2.0 * ghat[0, 0, 1:4]) and np.array_equal(g[..., 4:], ghat[..., 4:])
    assert g[0, 1, 0] == ghat[0, 1, 0] and np.array_equal(g[0, 1, 1:4], 0.5 * ghat[0, 1, 1:4])
    assert pc.amplification(pi)[0] == 2.0
    assert pc.amplification(pi[:, 1:])[0] == 1.0
