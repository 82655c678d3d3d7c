"""Pins of the CPU side of the step's reverse mode: the kernel's vector form (tests/step_vjp_check.joint_vjp_vector_form, the chain of
operations of mh_step_kernels.h: step_apply_t) against the transposed blocks of tests/step_derivatives_check.joint_blocks, the checker's
two contractions against each other, and ``chart_cotangent`` against the tangent map of (+) built from its definition.  No GPU."""
import numpy as np
import pytest
import torch

import step_derivatives_check as sc
import step_vjp_check as svc
from mecano_amd import autograd as mha
from mecano_amd import random_tools as rt
from test_dynamics_vjp_cpu import floating_mixed
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case

KINDS = {"revolute": mha.REVOLUTE, "prismatic": mha.PRISMATIC, "sixdof": mha.SIXDOF, "planar": mha.PLANAR, "spherical": mha.SPHERICAL}
STEPS = [0.1, 1.0e-3, 0.0, -0.05]


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("dt", STEPS)
def test_vector_form_is_the_transposed_blocks(kind, dt):
    """G_q^T g', G_v^T g', G_a^T g' of joint_blocks against the vector form, 200 random joint states and cotangents each:
    1e-13 max(1, |ref|_inf).  A fixed joint has no DoF and no block (integrate_vjp skips it: test below)."""
    t = KINDS[kind]
    k = mha._NDOF[t]
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(200):
        vj, aj = rng.uniform(-3.0, 3.0, k), rng.uniform(-30.0, 30.0, k)
        ga, gb = rng.uniform(-1.0, 1.0, k), rng.uniform(-1.0, 1.0, k)
        G, _ = sc.joint_blocks(t, dt, vj, aj)
        g = np.concatenate([ga, gb])
        for got, M in zip(svc.joint_vjp_vector_form(t, dt, vj, aj, ga, gb), G):
            ref = M.T @ g
            worst = max(worst, float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())))
    print(f"{kind} dt {dt}: vector form against the transposed blocks, worst relative error {worst:.3e}")
    assert worst <= 1.0e-13


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_vector_form_at_zero_step_is_exact(kind):
    t = KINDS[kind]
    k = mha._NDOF[t]
    rng = np.random.default_rng(18)
    vj, aj, ga, gb = (rng.uniform(-3.0, 3.0, k) for _ in range(4))
    gq, gqd, gqdd = svc.joint_vjp_vector_form(t, 0.0, vj, aj, ga, gb)
    assert np.array_equal(gq, ga) and np.array_equal(gqd, gb) and not gqdd.any()


@pytest.mark.parametrize("case", CASES + ["floating_mixed"])
def test_step_contraction_composes_the_integrator_and_the_forward_dynamics(case):
    """A^T g' and B^T g' against integrate_vjp around the checker's forward-dynamics matrices: gq = gq_int + Dq^T w, gqd = gqd_int + Dv^T w,
    gtau = Hinv^T w with w = gqdd_int -- the composition mh_aba_integrate_vjp_* makes.  Both sides are the same sums in another order:
    1e-11 max(1, |.|_inf).  Fixed joints and DoF indices no joint owns contribute nothing; a cotangent left out is a zero cotangent."""
    import dynamics_derivatives_check as dc
    sys_, desc = floating_mixed() if case == "floating_mixed" else make_case(case)
    B, dt = 3, 0.05
    q, qd, _, tau = rt.nextState(np.random.default_rng(5), sys_, B)
    rng = np.random.default_rng(8)
    ga, gb = rng.uniform(-1.0, 1.0, (B, desc.nv)), rng.uniform(-1.0, 1.0, (B, desc.nv))
    qdd, gq, gqd, gtau, sums, (Ainf, Binf) = svc.step_vjp(desc, dt, q, qd, tau, ga, gb, GRAVITY)
    qdd2, Dq, Dv, Hinv = dc.aba_derivatives(dc.DerivativeModel(desc), q, qd, tau, GRAVITY, None)
    assert np.array_equal(qdd, qdd2)
    iq, iv, w, isums = svc.integrate_vjp(desc, dt, qd, qdd, ga, gb)
    for got, ref, name in ((iq + np.einsum("bi,bij->bj", w, Dq), gq, "gq"), (iv + np.einsum("bi,bij->bj", w, Dv), gqd, "gqd"),
                           (np.einsum("bi,bij->bj", w, Hinv), gtau, "gtau")):
        assert np.abs(got - ref).max() <= 1.0e-11 * max(1.0, np.abs(ref).max()), name
    assert all((s >= 0.0).all() for s in sums + isums) and (Ainf >= 1.0 - 1e-12).all() and (Binf >= 0.0).all()
    only_a = svc.integrate_vjp(desc, dt, qd, qdd, ga, None)
    zero_b = svc.integrate_vjp(desc, dt, qd, qdd, ga, np.zeros_like(gb))
    assert all(np.array_equal(x, y) for x, y in zip(only_a[:3], zero_b[:3]))


def tangent_map(desc, q):
    """T [nq, nv] of one raw configuration from the definition of (+): d (q (+) dq) / d dq at dq = 0 -- columns Q o (e_k, 0) / 2 for a
    quaternion (raw, not normalised), R(Q / |Q|) e_k for a SixDoF translation, the rotation by the pitch for a planar one, 1 elsewhere."""
    m = sc._model(desc)
    T = np.zeros((m.nq, m.nv))
    for i in range(m.n):
        t, ci, di = int(m.type[i]), sc._cfg(m, i), m.dofs(i)
        if t in (mha.REVOLUTE, mha.PRISMATIC):
            T[ci[0], di[0]] = 1.0
        elif t == mha.PLANAR:
            c, s = np.cos(q[ci[0]]), np.sin(q[ci[0]])
            T[ci[0], di[0]] = 1.0
            T[ci[1], di[1]], T[ci[1], di[2]] = c, s
            T[ci[2], di[1]], T[ci[2], di[2]] = -s, c
        elif t in (mha.SPHERICAL, mha.SIXDOF):
            Q = q[ci[:4]]
            for k in range(3):
                e = np.zeros(4)
                e[k] = 1.0
                T[ci[:4], di[k]] = 0.5 * sc.quat_mul(Q, e)
            if t == mha.SIXDOF:
                from oracle import featherstone_np as fnp
                T[np.ix_(ci[4:7], di[3:6])] = fnp.quat_to_R(Q / np.linalg.norm(Q))
    return T


@pytest.mark.parametrize("case", ["floating_mixed", "humanoid30", "planar", "spherical", "arm7"])
def test_chart_cotangent_is_the_transposed_tangent_map(case):
    """T^T g_raw with non-unit quaternions among the inputs, and chart_cotangent(q, chart_pullback(q, g)) == g: 1e-14 max(1, |.|_inf)."""
    sys_, desc = floating_mixed() if case == "floating_mixed" else make_case(case)
    B = 4
    q = rt.nextState(np.random.default_rng(5), sys_, B)[0]
    maps = mha.chart_maps(desc)
    scale = np.random.default_rng(2).uniform(0.6, 1.7, (B, len(maps["quat_q"])))
    scale[0] = 1.0
    for k, rows in enumerate(maps["quat_q"]):
        q[:, rows] *= scale[:, k:k + 1]
    rng = np.random.default_rng(3)
    g_raw, g = rng.uniform(-1.0, 1.0, (B, desc.nq)), rng.uniform(-1.0, 1.0, (B, desc.nv))
    got = mha.chart_cotangent(desc, torch.from_numpy(q), torch.from_numpy(g_raw)).numpy()
    ref = np.stack([tangent_map(desc, q[b]).T @ g_raw[b] for b in range(B)])
    assert np.abs(got - ref).max() <= 1.0e-14 * max(1.0, np.abs(ref).max())
    back = mha.chart_cotangent(desc, torch.from_numpy(q), mha.chart_pullback(desc, torch.from_numpy(q), torch.from_numpy(g))).numpy()
    assert np.abs(back - g).max() <= 1.0e-14 * max(1.0, np.abs(g).max())
    with pytest.raises(ValueError):
        mha.chart_cotangent(desc, torch.from_numpy(q), torch.from_numpy(g_raw[:, :-1]))


def test_radial_passthrough_is_along_the_quaternion_only():
    """(g_Q' . Q') Q / |Q|^2 on the quaternions, zero elsewhere: for Q' = Q o D it is the gradient of g_Q' . Q' along Q."""
    sys_, desc = floating_mixed()
    rng = np.random.default_rng(4)
    q, qn, g = (torch.from_numpy(rng.normal(size=(3, desc.nq))) for _ in range(3))
    out = mha.radial_passthrough(desc, q, qn, g)
    maps = mha.chart_maps(desc)
    quat = sorted(i for r in maps["quat_q"] for i in r)
    assert not np.delete(out.numpy(), quat, axis=1).any()
    for rows in maps["quat_q"]:
        Q, D = q[0, rows].numpy(), sc.quat_exp(rng.normal(size=3))
        h = 1.0e-6
        f = lambda s: float(g[0, rows].numpy() @ sc.quat_mul(Q * s, D))
        qn1 = qn.clone()
        qn1[0, rows] = torch.from_numpy(sc.quat_mul(Q, D))
        r = mha.radial_passthrough(desc, q, qn1, g)[0, rows].numpy()
        assert abs(r @ Q - (f(1.0 + h) - f(1.0 - h)) / (2.0 * h)) <= 1.0e-8 * max(1.0, abs(r @ Q))
        assert np.abs(r - (r @ Q) / (Q @ Q) * Q).max() <= 1.0e-12 * max(1.0, np.abs(r).max())  # parallel to Q
