"""mh_rnea_vjp_* / mh_aba_vjp_* and the autograd functions on the device against the CPU checker (tests/dynamics_vjp_check.py: the
matrices of tests/dynamics_derivatives_check.py contracted with the cotangent, pinned by tests/test_dynamics_vjp_cpu.py) and against the
device's own neighbours (rnea_derivatives, aba_derivatives, aba, mass_matrix_inverse, gravity_gradient).

Bounds.  An output entry is a contraction sum_i u_i D_ij, so the project's per-entry bound of the matrix, TOL max(1, |D_ref|_inf)
(helpers.close), sums to |u|_1 TOL max(1, |D_ref|_inf) per configuration; gqdd takes H in place of D.  The forward form takes |w|_1 times
the per-row bound of helpers.close_aba as the forward-dynamics derivative tests apply it to the matrices: 8 sqrt(8 * 3 n) cond_inf(H) u
max(1, |D_ref|_inf), cond from the oracle's H.  fp32: helpers.f32_forward_tol(3 n) in place of TOL, u = 2^-24 in close_aba's form, the
checker fed the fp32-rounded inputs.  Every check records achieved / bound (helpers.record_parity)."""
import functools

import numpy as np
import pytest

import dynamics_vjp_check as vc
import helpers as hp
from helpers import DistinctRows, check_bad_outputs, close_aba, f32_aba_forward_factor, f32_forward_tol, group_cover, poisoned, record_parity
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu

TOL = 1.0e-10
AOS, SOA = 0, 1
U64, U32 = 2.0 ** -53, 2.0 ** -24
TREE_ROWS = np.array([0, 1, 31, 63, 64, 69])  # (the checker takes seconds per row of the 128-body tree)


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def soa(x):
    """[B, ...] -> [prod(...), B] contiguous"""
    return None if x is None else x.reshape(x.shape[0], -1).t().contiguous()


def host(t, layout):
    return None if t is None else (t.t() if layout == SOA else t).cpu().numpy().astype(np.float64)


def state(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)


def cotangent(B, nv, seed=8):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, nv))


def held(got, ref, bound, label, rows=None):
    """|got - ref|_inf <= bound per configuration; the worst achieved / bound goes to the parity log."""
    assert got.shape == ref.shape and not np.isnan(got).any(), label
    rows = np.arange(len(ref)) if rows is None else rows
    ratio = float((np.abs(got - ref).max(axis=1)[rows] / bound[rows]).max())
    record_parity(ratio, 1.0, label + " achieved / bound")
    assert ratio <= 1.0, f"{label}: achieved / bound = {ratio:.3e}"
    return ratio


def rnea_bounds(u, scales, tol=TOL):
    return [np.abs(u).sum(axis=1) * tol * np.maximum(1.0, s) for s in scales]


def aba_bounds(w, scales, conds, n_joints, unit):
    return [np.abs(w).sum(axis=1) * f32_aba_forward_factor(3 * n_joints) * conds * unit * np.maximum(1.0, s) for s in scales]


def conds_of(desc, q):
    return np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(q)])


def call(torch, method, arrays, f, layout, dtype=None, gravity=GRAVITY, **kw):
    """hm.rnea_vjp / hm.aba_vjp on host arrays (q, qd, qdd | tau, u | w): the outputs as AoS-shaped fp64 arrays."""
    args = [dev(torch, x, dtype) for x in arrays] + [dev(torch, f, dtype)]
    if layout == SOA:
        args = [soa(x) for x in args]
    out = method(args[0], args[1], args[2], args[3], gravity, args[4], layout, **kw)
    torch.cuda.synchronize()
    return tuple(host(t, layout) for t in out)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("wrenches", ["none", "random"])
def test_fp64_matches_checker(torch_cuda, case, layout, wrenches):
    """Every model of the derivative tests, both layouts, without and with wrenches; 70 states: one full wave and a ragged one, split
    over several waves per group (the parts of small batches)."""
    from mecano_amd.engine import HipModel
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q, qd, qdd, _ = state(sys_, B)
    u = cotangent(B, desc.nv)
    f = None if wrenches == "none" else random_wrenches(np.random.default_rng(21), B, desc.n_joints)
    got = call(torch_cuda, hm.rnea_vjp, (q, qd, qdd, u), f, layout)
    *ref, scales = vc.rnea_vjp(desc, q, qd, qdd, u, GRAVITY, f)
    for g, r, b, name in zip(got, ref, rnea_bounds(u, scales), ("gq", "gqd", "gqdd")):
        held(g, r, b, name)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("wrenches", ["none", "random"])
def test_forward_fp64_matches_checker(torch_cuda, case, layout, wrenches):
    from mecano_amd.engine import HipModel
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q, qd, _, tau = state(sys_, B)
    w = cotangent(B, desc.nv, 9)
    f = None if wrenches == "none" else random_wrenches(np.random.default_rng(31), B, desc.n_joints)
    qdd, *got = call(torch_cuda, hm.aba_vjp, (q, qd, tau, w), f, layout)
    qdd_ref, *ref, scales = vc.aba_vjp(desc, q, qd, tau, w, GRAVITY, f)
    conds = conds_of(desc, q)
    close_aba(qdd, qdd_ref, None, desc.n_joints, U64, label="qdd", conds=conds)
    for g, r, b, name in zip(got, ref, aba_bounds(w, scales, conds, desc.n_joints, U64), ("gq", "gqd", "gtau")):
        held(g, r, b, name)


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_fp32_matches_checker(torch_cuda, case):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q, qd, qdd, tau = (x.astype(np.float32) for x in state(sys_, B))
    u = cotangent(B, desc.nv).astype(np.float32)
    f = random_wrenches(np.random.default_rng(22), B, desc.n_joints).astype(np.float32)
    q64, qd64, qdd64, tau64, u64, f64 = (x.astype(np.float64) for x in (q, qd, qdd, tau, u, f))
    *ref, scales = vc.rnea_vjp(desc, q64, qd64, qdd64, u64, GRAVITY, f64)
    qdd_ref, *ref_f, scales_f = vc.aba_vjp(desc, q64, qd64, tau64, u64, GRAVITY, f64)
    conds = conds_of(desc, q64)
    for layout in (AOS, SOA):
        got = call(torch, hm.rnea_vjp, (q, qd, qdd, u), f, layout, dtype=torch.float32)
        for g, r, b, name in zip(got, ref, rnea_bounds(u64, scales, f32_forward_tol(3 * desc.n_joints)), ("gq", "gqd", "gqdd")):
            held(g, r, b, f"fp32 {name} layout {layout}")
        qdd_d, *got = call(torch, hm.aba_vjp, (q, qd, tau, u), f, layout, dtype=torch.float32)
        close_aba(qdd_d, qdd_ref, None, desc.n_joints, U32, label=f"fp32 qdd layout {layout}", conds=conds)
        for g, r, b, name in zip(got, ref_f, aba_bounds(u64, scales_f, conds, desc.n_joints, U32), ("gq", "gqd", "gtau")):
            held(g, r, b, f"fp32 forward {name} layout {layout}")


def test_tree128_rows(torch_cuda):
    """The committed 128-body benchmark tree, nv = 323, fp64 AoS: both calls on the rows TREE_ROWS; every row free of NaN."""
    from mecano_amd.engine import HipModel
    sys_ = rt.committedBenchmarkSystems()["tree128"]
    desc = sys_.toModelDesc()
    assert desc.nv == 323
    hm, B = HipModel(desc), 70
    q, qd, qdd, tau = state(sys_, B)
    u = cotangent(B, desc.nv)
    f = random_wrenches(np.random.default_rng(22), B, desc.n_joints)
    got = call(torch_cuda, hm.rnea_vjp, (q, qd, qdd, u), f, AOS)
    *ref, scales = vc.rnea_vjp(desc, q, qd, qdd, u, GRAVITY, f, rows=TREE_ROWS)
    for g, r, b, name in zip(got, ref, rnea_bounds(u, scales), ("gq", "gqd", "gqdd")):
        held(g, r, b, "tree128 " + name, rows=TREE_ROWS)
    qdd_d, *got = call(torch_cuda, hm.aba_vjp, (q, qd, tau, u), f, AOS)
    qdd_ref, *ref, scales = vc.aba_vjp(desc, q, qd, tau, u, GRAVITY, f, rows=TREE_ROWS)
    conds = np.ones(B)
    conds[TREE_ROWS] = conds_of(desc, q[TREE_ROWS])
    close_aba(qdd_d[TREE_ROWS], qdd_ref[TREE_ROWS], None, desc.n_joints, U64, label="tree128 qdd", conds=conds[TREE_ROWS])
    for g, r, b, name in zip(got, ref, aba_bounds(u, scales, conds, desc.n_joints, U64), ("gq", "gqd", "gtau")):
        held(g, r, b, "tree128 forward " + name, rows=TREE_ROWS)


# ------------------------------------------------------------------------------------------------ device against device
@pytest.mark.parametrize("case", ["humanoid30", "planar", "spherical"])
def test_contracts_the_device_matrices(torch_cuda, case):
    """For random v with |v|_inf <= 1: gq . v = u^T (D v) with D from rnea_derivatives / aba_derivatives on the same inputs, within the
    parity bound; qdd_out is hm.aba and gtau is mass_matrix_inverse(q) w within close_aba."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B, nv = HipModel(desc), 70, desc.nv
    qh, qdh, qddh, tauh = state(sys_, B)
    uh, vh = cotangent(B, nv), cotangent(B, nv, 12)
    q, qd, qdd, tau, u, v = (dev(torch, x) for x in (qh, qdh, qddh, tauh, uh, vh))
    f = dev(torch, random_wrenches(np.random.default_rng(23), B, desc.n_joints))
    conds = conds_of(desc, qh)
    gq, gqd, _ = hm.rnea_vjp(q, qd, qdd, u, GRAVITY, f)
    _, Dq, Dv = hm.rnea_derivatives(q, qd, qdd, GRAVITY, f)
    scales = [D.abs().amax(dim=(1, 2)).cpu().numpy() for D in (Dq, Dv)]
    for g, D, b, name in zip((gq, gqd), (Dq, Dv), rnea_bounds(uh, scales), ("gq", "gqd")):
        lhs = (g * v).sum(1, keepdim=True).cpu().numpy()
        rhs = torch.einsum("bi,bij,bj->b", u, D, v)[:, None].cpu().numpy()
        held(lhs, rhs, b, name + " . v against u^T (D v)")
    qdd_v, gq, gqd, gtau = hm.aba_vjp(q, qd, tau, u, GRAVITY, f)
    _, Dq, Dv, Hinv = hm.aba_derivatives(q, qd, tau, GRAVITY, f)
    scales = [D.abs().amax(dim=(1, 2)).cpu().numpy() for D in (Dq, Dv)]
    for g, D, b, name in zip((gq, gqd), (Dq, Dv), aba_bounds(uh, scales, conds, desc.n_joints, U64), ("gq", "gqd")):
        lhs = (g * v).sum(1, keepdim=True).cpu().numpy()
        rhs = torch.einsum("bi,bij,bj->b", u, D, v)[:, None].cpu().numpy()
        held(lhs, rhs, b, "forward " + name + " . v against w^T (D v)")
    close_aba(qdd_v.cpu().numpy(), hm.aba(q, qd, tau, GRAVITY, f).cpu().numpy(), None, desc.n_joints, U64, label="qdd vs aba", conds=conds)
    ref = torch.einsum("bij,bj->bi", hm.mass_matrix_inverse(q), u).cpu().numpy()
    close_aba(gtau.cpu().numpy(), ref, None, desc.n_joints, U64, label="gtau vs mass_matrix_inverse", conds=conds)


# ------------------------------------------------------------------------------------------------ exact cases
def test_exact_zeros_and_the_gravity_gradient(torch_cuda):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 100
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    uh = cotangent(B, desc.nv)
    u, z = dev(torch, uh), torch.zeros_like(qd)
    f = dev(torch, random_wrenches(np.random.default_rng(25), B, desc.n_joints, always=True))
    for layout in (AOS, SOA):
        a = (q, qd, qdd, u, z, tau, f) if layout == AOS else tuple(soa(x) for x in (q, qd, qdd, u, z, tau, f))
        assert not any(t.any() for t in hm.rnea_vjp(a[0], a[1], a[2], a[4], GRAVITY, a[6], layout))           # u = 0
        assert not any(t.any() for t in hm.aba_vjp(a[0], a[1], a[5], a[4], GRAVITY, a[6], layout)[1:])        # w = 0
        off = hm.rnea_vjp(a[0], None, a[2], a[3], GRAVITY, a[6], layout, consider_coriolis=False)
        ref = hm.rnea_vjp(a[0], a[4], a[2], a[3], GRAVITY, a[6], layout)
        assert all(torch.equal(x, y) for x, y in zip(off, ref)) and not off[1].any() and off[0].any()
        off = hm.rnea_vjp(a[0], a[1], None, a[3], GRAVITY, a[6], layout, consider_accelerations=False)
        ref = hm.rnea_vjp(a[0], a[1], a[4], a[3], GRAVITY, a[6], layout)
        assert all(torch.equal(x, y) for x, y in zip(off, ref))
    for fe in (None, f):  # at rest: u^T (gravity gradient)
        gq = hm.rnea_vjp(q, z, z, u, GRAVITY, fe)[0].cpu().numpy()
        grad = hm.gravity_gradient(q, GRAVITY, fe)[1]
        ref = torch.einsum("bi,bij->bj", u, grad).cpu().numpy()
        held(gq, ref, rnea_bounds(uh, [grad.abs().amax(dim=(1, 2)).cpu().numpy()])[0], "at rest vs gravity_gradient")


def test_unowned_dof_indices_get_zeros(torch_cuda):
    """A custom index map with two DoF / configuration indices no joint owns: zeros there, the default map's values elsewhere."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, d0 = make_case("onedof_tree")
    B, nv = 70, d0.nv
    q, qd, qdd, tau = state(sys_, B)
    u = cotangent(B, nv)
    place = np.array([k + (k >= 3) + (k >= 7) for k in range(nv)])  # indices 3 and 8 of the wide map stay free
    free = np.setdiff1d(np.arange(nv + 2), place)
    d1 = sys_.toModelDesc()
    d1.dof_indices = place[np.asarray(d0.dof_indices)].astype(np.int32)
    d1.cfg_indices = place[np.asarray(d0.cfg_indices)].astype(np.int32)
    d1.nv = d1.nq = nv + 2
    wide = lambda x: np.ascontiguousarray(np.insert(np.insert(x, 3, 0.25, axis=1), 8, -0.5, axis=1))
    assert np.array_equal(wide(q)[:, place], q)
    h0, h1 = HipModel(d0), HipModel(d1)
    base = call(torch, h0.rnea_vjp, (q, qd, qdd, u), None, AOS)
    _, *ref_f, scales = vc.aba_vjp(d0, q, qd, tau, u, GRAVITY)
    bounds = aba_bounds(u, scales, conds_of(d0, q), d0.n_joints, U64)
    for layout in (AOS, SOA):
        outs_i = tuple(poisoned(torch, B, (nv + 2,), torch.float64)[0] if layout == AOS else poisoned(torch, nv + 2, (B,), torch.float64)[0] for _ in range(3))
        outs_f = tuple(poisoned(torch, B, (nv + 2,), torch.float64)[0] if layout == AOS else poisoned(torch, nv + 2, (B,), torch.float64)[0] for _ in range(4))
        got = call(torch, h1.rnea_vjp, tuple(wide(x) for x in (q, qd, qdd, u)), None, layout, out=outs_i)
        got += call(torch, h1.aba_vjp, tuple(wide(x) for x in (q, qd, tau, u)), None, layout, out=outs_f)[1:]
        for k, g in enumerate(got):
            assert not np.isnan(g).any() and not g[:, free].any(), f"output {k}"
            if k < 3:  # the same kernel on the same numbers
                assert np.array_equal(g[:, place], base[k]), f"output {k}"
            else:
                held(g[:, place], ref_f[k - 3], bounds[k - 3], f"forward output {k - 3}, wide map")


# ------------------------------------------------------------------------------------------------ scattered index maps
@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    """States and cotangents in the identity description's index space and the checker's outputs on them: once per model and precision,
    shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if dtype_name == "float32" else np.float64
    q, qd, qdd, tau = DistinctRows(sys_, 16, seed=51).rows(np.arange(70), np_dt)
    u = cotangent(70, d0.nv, 52).astype(np_dt).astype(np.float64)
    f = random_wrenches(np.random.default_rng(53), 70, d0.n_joints).astype(np_dt).astype(np.float64)
    conds = conds_of(d0, q)
    assert conds.max() < 1.0e8
    return (q, qd, qdd, tau, u, f), vc.rnea_vjp(d0, q, qd, qdd, u, GRAVITY, f), vc.aba_vjp(d0, q, qd, tau, u, GRAVITY, f), conds


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """rnea_vjp and aba_vjp on a description whose maps send every DoF and every configuration entry somewhere else (with holes: two
    indices of each space owned by no joint, holding 7.0 in every input, the cotangent included), against the checker on the IDENTITY
    description: the cotangent goes in and every gradient comes back through the DoF map and meets this file's bounds (rnea_bounds /
    aba_bounds, close_aba for qdd); the gradients at unowned indices are exact zeros, the guard rows stay poisoned; each gradient asked
    for alone (the other outputs NULL) meets the same bound; read without moving them back the outputs miss the
    reference by more than 1e-3."""
    torch = torch_cuda
    dtype, unit = getattr(torch, dtype_name), (U32 if dtype_name == "float32" else U64)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, n = hp.scattered_model(d, model), 70, d.nv, d0.n_joints
    (q, qd, qdd, tau, u, f), inv, fwd, conds = _scattered_reference(model, dtype_name)
    is_soa = layout == SOA
    lay = soa if is_soa else (lambda x: x)
    tq, tqd, tqdd, ttau, tu = (lay(dev(torch, x, dtype)) for x in
                               (hp.to_q(q, pq, d.nq), hp.to_v(qd, pv, nv), hp.to_v(qdd, pv, nv), hp.to_v(tau, pv, nv), hp.to_v(u, pv, nv)))
    tf = lay(dev(torch, f, dtype))
    *ref_i, scales_i = inv
    qdd_ref, *ref_f, scales_f = fwd
    bounds_i = rnea_bounds(u, scales_i, TOL if dtype_name == "float64" else f32_forward_tol(3 * n))
    bounds_f = aba_bounds(u, scales_f, conds, n, unit)

    def run(method, x3, places, want):
        outs, guards = hp.poisoned_set(torch, B, [(nv,)] * places, dtype, is_soa)
        outs = [o if k in want else None for k, o in enumerate(outs)]
        method(tq, tqd, x3, tu, GRAVITY, tf, layout, out=tuple(outs))
        torch.cuda.synchronize()
        hp.guards_intact([g for k, g in enumerate(guards) if k in want], method.__name__)
        return [None if o is None else hp.rows_of(o, B, (nv,), is_soa) for o in outs]

    got = run(hm.rnea_vjp, tqdd, 3, (0, 1, 2))
    for k, (g, r, b, name) in enumerate(zip(got, ref_i, bounds_i, ("gq", "gqd", "gqdd"))):
        back, free = hp.from_v(g, pv)
        assert not free.any(), name  # exact zeros, and written
        held(back, r, b, f"scattered {name}")
        hp.assert_misses(hp.keep_order(g, pv), r, name)
        alone = hp.from_v(run(hm.rnea_vjp, tqdd, 3, (k,))[k], pv)
        assert not alone[1].any(), name
        held(alone[0], r, b, f"scattered {name} alone")
    got = run(hm.aba_vjp, ttau, 4, (0, 1, 2, 3))
    close_aba(hp.from_v(got[0], pv)[0], qdd_ref, None, n, unit, label="scattered qdd", conds=conds)
    for k, (g, r, b, name) in enumerate(zip(got[1:], ref_f, bounds_f, ("gq", "gqd", "gtau")), start=1):
        back, free = hp.from_v(g, pv)
        assert not free.any(), name
        held(back, r, b, f"scattered forward {name}")
        hp.assert_misses(hp.keep_order(g, pv), r, "forward " + name)
        alone = hp.from_v(run(hm.aba_vjp, ttau, 4, (k,))[k], pv)
        assert not alone[1].any(), name
        held(alone[0], r, b, f"scattered forward {name} alone")


# ------------------------------------------------------------------------------------------------ cover of batches
def _cover_case(torch, sys_, desc, B, grid, layout, with_f, skip=None, forward=False):
    """B distinct rows, poisoned outputs with a guard row behind them, every row group checked against the checker; `skip`: index of
    the output passed as NULL."""
    from mecano_amd.engine import HipModel
    hm = HipModel(desc)
    rows = DistinctRows(sys_, 256, seed=29)
    q, qd, qdd, tau = rows.device(torch, B)
    idx = group_cover(B, grid)
    nv = desc.nv
    u_host = cotangent(64, nv, 13)
    f_host = random_wrenches(np.random.default_rng(24), 64, desc.n_joints) if with_f else None
    period = torch.arange(B, device="cuda") % 64
    u = dev(torch, u_host)[period].contiguous()
    f = dev(torch, f_host)[period].contiguous() if with_f else None
    outs, guards = [], []
    for k in range(4 if forward else 3):
        if k in (skip if isinstance(skip, tuple) else (skip,)):
            outs.append(None), guards.append(None)
            continue
        o, g = poisoned(torch, B, (nv,), torch.float64) if layout == AOS else poisoned(torch, nv, (B,), torch.float64)
        outs.append(o), guards.append(g)
    x3 = tau if forward else qdd
    args = (q, qd, x3, u, GRAVITY, f) if layout == AOS else (soa(q), soa(qd), soa(x3), soa(u), GRAVITY, soa(f))
    (hm.aba_vjp if forward else hm.rnea_vjp)(*args, layout, out=tuple(outs))
    torch.cuda.synchronize()
    qi, qdi, qddi, taui = rows.rows(idx)
    ui, fi = u_host[idx % 64], None if f_host is None else f_host[idx % 64]
    if forward:
        conds = conds_of(desc, qi)
        qdd_ref, *ref, scales = vc.aba_vjp(desc, qi, qdi, taui, ui, GRAVITY, fi)
        ref, bounds = [qdd_ref] + ref, [None] + aba_bounds(ui, scales, conds, desc.n_joints, U64)
    else:
        *ref, scales = vc.rnea_vjp(desc, qi, qdi, qddi, ui, GRAVITY, fi)
        bounds = rnea_bounds(ui, scales)
    take = torch.as_tensor(idx, device="cuda")
    for k, (o, g, r, b) in enumerate(zip(outs, guards, ref, bounds)):
        if o is None:
            continue
        assert torch.isnan(g).all(), f"output {k}: wrote past the last row"
        assert not torch.isnan(o).any(), f"output {k}: rows left unwritten (NaN)"
        got = (o if layout == AOS else o.t())[take].cpu().numpy()
        if b is None:
            close_aba(got, r, None, desc.n_joints, U64, label="qdd", conds=conds)
        else:
            held(got, r, b, f"output {k}")


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the grid holds (8 per CU), plus a ragged last group: every lane loops over several groups of 64."""
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    sys_, desc = make_case("arm7")
    _cover_case(torch, sys_, desc, 2 * 8 * cus * 64 + 64 + 37, 8 * cus, layout, with_f=True)


@pytest.mark.parametrize("case,B", [("humanoid30", 8192 + 37), ("onedof_tree", 4096), ("humanoid30", 64 * 3 + 1)])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_ragged_and_full_batches_cover_every_row_group(torch_cuda, case, B, layout):
    """(The parts split is taken at 64 * 3 + 1.)  The forward form is two launches of mh_aba_*, whose own tests cover their row groups,
    and this kernel: its cover runs at 64 * 5 + 3 below."""
    sys_, desc = make_case(case)
    _cover_case(torch_cuda, sys_, desc, B, None, layout, with_f=(B % 2 == 1))


@pytest.mark.parametrize("skip", [0, 1, 2])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_each_output_null_in_turn(torch_cuda, skip, layout):
    sys_, desc = make_case("humanoid30")
    _cover_case(torch_cuda, sys_, desc, 64 * 5 + 3, None, layout, with_f=True, skip=skip)


@pytest.mark.parametrize("skip", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_each_output_null_in_turn(torch_cuda, skip, layout):
    sys_, desc = make_case("humanoid30")
    _cover_case(torch_cuda, sys_, desc, 64 * 5 + 3, None, layout, with_f=True, skip=skip, forward=True)


@pytest.mark.parametrize("skip", [(0, 1, 2), (1, 2), (0, 3)])
@pytest.mark.parametrize("case,B", [("arm7", 1), ("arm7", 65), ("humanoid30", 197)])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_outputs_null_together(torch_cuda, skip, case, B, layout):
    """gtau alone (no qdd is needed: the first forward-dynamics launch is skipped), qdd and gtau without gq and gqd (no adjoint launch),
    and gq and gqd with qdd and H^-1 w both in the context's scratch."""
    sys_, desc = make_case(case)
    _cover_case(torch_cuda, sys_, desc, B, None, layout, with_f=True, skip=skip, forward=True)


@pytest.mark.parametrize("case,B", [("arm7", 1), ("arm7", 65), ("humanoid30", 197)])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_fp32_outputs_null_together(torch_cuda, case, B, layout):
    """The same selections in fp32: what is asked for has the bits of the call that asks for everything, which
    test_fp32_matches_checker holds to the checker."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm = HipModel(desc)
    put = lambda x: dev(torch, x.reshape(B, -1), torch.float32) if layout == AOS else soa(dev(torch, x.reshape(B, -1), torch.float32))
    q, qd, _, tau = (put(x) for x in state(sys_, B))
    w, f = put(cotangent(B, desc.nv, 9)), put(random_wrenches(np.random.default_rng(31), B, desc.n_joints))
    full = hm.aba_vjp(q, qd, tau, w, GRAVITY, f, layout)
    assert all(torch.isfinite(t).all() for t in full)
    for keep in ((3,), (0, 3), (1, 2)):  # of (qdd, gq, gqd, gtau)
        outs = tuple(torch.full_like(t, float("nan")) if k in keep else None for k, t in enumerate(full))
        res = hm.aba_vjp(q, qd, tau, w, GRAVITY, f, layout, out=outs)
        torch.cuda.synchronize()
        assert all((r is None) if k not in keep else torch.equal(r, full[k]) for k, r in enumerate(res)), keep


@pytest.mark.parametrize("case,B", [("arm7", 65), ("humanoid30", 197)])
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_form_hands_the_callers_switches_to_forward_dynamics_only(torch_cuda, case, B, dtype_name, layout):
    """mh_aba_vjp_* handed consider_coriolis = 0 through the C ABI (the engine never does).  The first launch is mh_aba_* with the
    caller's options: qdd_out has the bits of mh_aba_* with the same options.  gtau is H^-1 w, within the bounds of the call with the
    switch on.  The adjoint sweep runs with both switches on at that qdd: gq and gqd have the bits of -mh_rnea_vjp_*(q, qd, qdd_out,
    u = gtau) with the switches on, and gqd is not the zeros a sweep with the switch off stores."""
    import ctypes

    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    dtype, unit, sfx = (torch.float64, U64, "f64") if dtype_name == "float64" else (torch.float32, U32, "f32")
    sys_, desc = make_case(case)
    hm = HipModel(desc)
    q, qd, _, tau = (x.astype(dtype_name) for x in state(sys_, B))
    w = cotangent(B, desc.nv, 9).astype(dtype_name)
    f = random_wrenches(np.random.default_rng(31), B, desc.n_joints).astype(dtype_name)
    put = lambda x: dev(torch, x.reshape(B, -1), dtype) if layout == AOS else soa(dev(torch, x.reshape(B, -1), dtype))
    tq, tqd, ttau, tf, tw = (put(x) for x in (q, qd, tau, f, w))
    qdd, gq, gqd, gtau, qdd_aba = (torch.full_like(tw, float("nan")) for _ in range(5))
    g, ra = hm._root(GRAVITY)
    opts = hm._options(layout, False, True, torch.cuda.current_stream().cuda_stream, root_acceleration=ra)
    lib = _lib.load()
    _lib.check(getattr(lib, "mh_aba_vjp_" + sfx)(hm._h, B, tq.data_ptr(), tqd.data_ptr(), ttau.data_ptr(), g, tf.data_ptr(), tw.data_ptr(),
                                                 ctypes.byref(opts), qdd.data_ptr(), gq.data_ptr(), gqd.data_ptr(), gtau.data_ptr()))
    _lib.check(getattr(lib, "mh_aba_" + sfx)(hm._h, B, tq.data_ptr(), tqd.data_ptr(), ttau.data_ptr(), g, tf.data_ptr(), ctypes.byref(opts),
                                             qdd_aba.data_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(qdd).all() and torch.equal(qdd, qdd_aba)
    ref = hm.rnea_vjp(tq, tqd, qdd, gtau, GRAVITY, tf, layout)
    torch.cuda.synchronize()
    assert torch.equal(gq, -ref[0]) and torch.equal(gqd, -ref[1]) and gqd.any()
    q64, qd64, tau64, w64, f64 = (x.astype(np.float64) for x in (q, qd, tau, w, f))
    conds = conds_of(desc, q64)
    mu_ref = np.linalg.solve(OracleModel(desc).crba(q64), w64[:, :, None])[:, :, 0]
    close_aba(host(gtau, layout), mu_ref, None, desc.n_joints, unit, label="switch off: gtau", conds=conds)


# ------------------------------------------------------------------------------------------------ plumbing
def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() and a first call both calls are
    captured into a graph (they allocate nothing) and the replay gives the bits of the direct call, also on changed inputs."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 1000
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    u = dev(torch, cotangent(B, desc.nv))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    ref_i = hm.rnea_vjp(q, qd, qdd, u, GRAVITY, f)
    ref_f = hm.aba_vjp(q, qd, tau, u, GRAVITY, f)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    out_i = tuple(torch.empty_like(t) for t in ref_i)
    out_f = tuple(torch.empty_like(t) for t in ref_f[1:3])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view.rnea_vjp(q, qd, qdd, u, GRAVITY, f, out=out_i)
        view.aba_vjp(q, qd, tau, u, GRAVITY, f, out=(None, out_f[0], out_f[1], None))  # qdd and H^-1 w in the context's scratch
        view.check(s.cuda_stream)
        assert all(torch.equal(a, b) for a, b in zip(out_i, ref_i)) and all(torch.equal(a, b) for a, b in zip(out_f, ref_f[1:3]))
        for t in out_i + out_f:
            t.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            view.rnea_vjp(q, qd, qdd, u, GRAVITY, f, out=out_i)
            view.aba_vjp(q, qd, tau, u, GRAVITY, f, out=(None, out_f[0], out_f[1], None))
    torch.cuda.synchronize()
    assert not any(t.any() for t in out_i + out_f)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out_i, ref_i)) and all(torch.equal(a, b) for a, b in zip(out_f, ref_f[1:3]))
    q2, u2 = dev(torch, state(sys_, B, seed=6)[0]), dev(torch, cotangent(B, desc.nv, 14))
    ref_i2 = hm.rnea_vjp(q2, qd, qdd, u2, GRAVITY, f)
    ref_f2 = hm.aba_vjp(q2, qd, tau, u2, GRAVITY, f)
    q.copy_(q2), u.copy_(u2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out_i, ref_i2)) and all(torch.equal(a, b) for a, b in zip(out_f, ref_f2[1:3]))
    view.close()


def test_wrong_shapes_overlaps_and_source_joints_are_refused(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = HipModel(desc), 10, desc.nv, desc.n_joints
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    u = dev(torch, cotangent(B, nv))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(B, n, 5), z(n * 6, B)):
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_vjp(q, qd, qdd, u, GRAVITY, bad_f)
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_vjp(q, qd, tau, u, GRAVITY, bad_f)
    for bad_out in ((z(B, nv + 1), None, None), (None, z(nv, B), None), (None, None, None), (None, z(B, nv))):
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_vjp(q, qd, qdd, u, GRAVITY, None, out=bad_out)
    for bad_out in ((z(B, nv), None, None, None), (None, z(B, nv + 1), None, None), (None, z(B, nv), None)):
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_vjp(q, qd, tau, u, GRAVITY, None, out=bad_out)
    vec = (B, nv)
    check_bad_outputs(torch, [vec, vec, vec], lambda out: hm.rnea_vjp(q, qd, qdd, u, GRAVITY, None, out=out))
    check_bad_outputs(torch, [vec, vec, vec, vec], lambda out: hm.aba_vjp(q, qd, tau, u, GRAVITY, None, out=out))
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_vjp(q, qd, qdd, z(B, nv + 1), GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_vjp(q, qd, None, u, GRAVITY)
    # every forbidden overlap: an output on an input (q has nq = nv here), two outputs on each other -- nothing is written
    nan = lambda: torch.full((B, nv), float("nan"), dtype=torch.float64, device="cuda")
    for name, inputs, n_out in (("rnea_vjp", (q, qd, qdd, u), 3), ("aba_vjp", (q, qd, tau, u), 4)):
        method = getattr(hm, name)
        before = [t.clone() for t in inputs]
        for k in range(n_out):
            for t in inputs:
                outs = [nan() for _ in range(n_out)]
                outs[k] = t
                with pytest.raises(_lib.MecanoHipError):
                    method(*inputs, GRAVITY, None, out=tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for j, o in enumerate(outs) if j != k)
            for j in range(k):
                outs = [nan() for _ in range(n_out)]
                outs[k] = outs[j]
                with pytest.raises(_lib.MecanoHipError):
                    method(*inputs, GRAVITY, None, out=tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for o in outs)
        assert all(torch.equal(a, b) for a, b in zip(inputs, before))
    modes = [0] * n
    modes[2] = 1
    hm.set_joint_source_modes(modes)
    for method, x3 in ((hm.rnea_vjp, qdd), (hm.aba_vjp, tau)):
        with pytest.raises(_lib.MecanoHipError):
            method(q, qd, x3, u, GRAVITY)
    hm.set_joint_source_modes(None)


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_is_the_vjp_call_plus_the_pullback(torch_cuda):
    """humanoid30 (floating root), B = 70, fp64: torch.autograd.grad of sum(w * f(...)) is hm.*_vjp plus chart_pullback bit for bit and
    the checker's contraction within the parity bound; an input that does not require a gradient yields None and its output is not
    computed; a second backward raises."""
    from mecano_amd import autograd as mha
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 70
    qh, qdh, qddh, tauh = state(sys_, B)
    wh = cotangent(B, desc.nv, 9)
    w = dev(torch, wh)
    conds = conds_of(desc, qh)
    for fn, vjp, check, x3h in ((mha.aba, hm.aba_vjp, vc.aba_vjp, tauh), (mha.rnea, hm.rnea_vjp, vc.rnea_vjp, qddh)):
        q, qd, x3 = (dev(torch, x).requires_grad_() for x in (qh, qdh, x3h))
        out = fn(hm, q, qd, x3, GRAVITY, None)
        got = torch.autograd.grad((w * out).sum(), (q, qd, x3))
        direct = vjp(q.detach(), qd.detach(), x3.detach(), w, GRAVITY)[-3:]
        assert torch.equal(got[0], hm.chart_pullback(q.detach(), direct[0])) and torch.equal(got[1], direct[1]) and torch.equal(got[2], direct[2])
        *ref, scales = check(desc, qh, qdh, x3h, wh, GRAVITY)
        bounds = rnea_bounds(wh, scales) if fn is mha.rnea else aba_bounds(wh, scales, conds, desc.n_joints, U64)
        for g, r, b, name in zip(direct, ref[-3:], bounds, ("gq", "gqd", "g3")):
            held(g.cpu().numpy(), r, b, f"{fn.__name__} {name}")
        # only qd asks: the others come back as None, and the call is made with their outputs NULL
        q, qd, x3 = dev(torch, qh), dev(torch, qdh).requires_grad_(), dev(torch, x3h)
        seen = {}
        name = vjp.__name__
        setattr(hm, name, lambda *a, _v=vjp, **kw: (seen.update(out=kw["out"]), _v(*a, **kw))[1])
        try:
            loss = (w * fn(hm, q, qd, x3, GRAVITY, None)).sum()
            (gqd,) = torch.autograd.grad(loss, (qd,), create_graph=True)
        finally:
            delattr(hm, name)
        assert torch.equal(gqd, direct[1])
        assert [t is None for t in seen["out"]][-3:] == [True, False, True]
        with pytest.raises(RuntimeError):
            gqd.sum().backward()
