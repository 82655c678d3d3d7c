"""mh_integrate_vjp_* / mh_aba_integrate_vjp_* and autograd.integrate / autograd.step on the device against the CPU checker
(tests/step_vjp_check.py: the transposed matrices of tests/step_derivatives_check.py applied to the cotangents, pinned by
tests/test_step_vjp_cpu.py).  The reference is the checker only, never the code under test.

Bounds.  mh_integrate_vjp_*: per ENTRY 24 u x the sum of the absolute terms of that entry (|G|_abs^T |g'|), the factor
tests/test_gpu_step_derivatives.py takes for the same blocks applied forwards; an entry with a zero bound is exactly zero.
mh_aba_integrate_vjp_*: per configuration |g'|_1 f32_aba_forward_factor(3 n + 1) cond_inf(H) u max(1, |A_ref|_inf) on (gq, gqd) and the
same with |B_ref|_inf on gtau -- aba_bounds of tests/test_gpu_dynamics_vjp.py with the one more combination step of the step
linearisation's test; qdd by helpers.close_aba.  fp32: u = 2^-24, the checker fed the fp32-rounded inputs.  Every check records
achieved / bound (helpers.record_parity)."""
import functools

import numpy as np
import pytest

import helpers as hp
import step_vjp_check as svc
from helpers import DistinctRows, check_bad_outputs, close_aba, f32_aba_forward_factor, group_cover, poisoned, record_parity
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu

AOS, SOA = 0, 1
U64, U32 = 2.0 ** -53, 2.0 ** -24
B70 = 70  # one full wave and a ragged one


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


def cotangents(B, nv, seed=8):
    r = np.random.default_rng(seed)
    return r.uniform(-1.0, 1.0, (B, nv)), r.uniform(-1.0, 1.0, (B, nv))


def conds_of(desc, q):
    return np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(q)])


def lay(t, layout):
    return t if layout == AOS or t is None else soa(t)


def run_integrate(torch, hm, dt, qd, qdd, ga, gb, layout, dtype=None, **kw):
    """hm.integrate_vjp on host arrays: (gq, gqd, gqdd) as AoS-shaped fp64 arrays."""
    a = [lay(dev(torch, x, dtype), layout) for x in (qd, qdd, ga, gb)]
    out = hm.integrate_vjp(dt, a[0], a[1], a[2], a[3], layout, **kw)
    torch.cuda.synchronize()
    return tuple(host(t, layout) for t in out)


def run_step(torch, hm, dt, q, qd, tau, ga, gb, f, layout, dtype=None, **kw):
    """hm.step_vjp on host arrays: (qdd, gq, gqd, gtau) as AoS-shaped fp64 arrays."""
    a = [lay(dev(torch, x, dtype), layout) for x in (q, qd, tau, ga, gb, f)]
    out = hm.step_vjp(dt, a[0], a[1], a[2], a[3], a[4], GRAVITY, a[5], layout, **kw)
    torch.cuda.synchronize()
    return tuple(host(t, layout) for t in out)


def held_entries(got, ref, abs_sum, unit, label, extra=None):
    """|got - ref| <= 24 u abs_sum (+ extra) entry by entry, entries with a zero bound exactly zero; worst achieved / bound is logged."""
    assert got.shape == ref.shape and not np.isnan(got).any(), label
    bound = 24.0 * unit * abs_sum + (0.0 if extra is None else extra)
    zero = bound == 0.0
    assert not got[zero].any(), f"{label}: an entry with a zero bound is not zero"
    err = np.abs(got - ref)
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f"{label}: worst err / bound = {ratio:.3e}")
    record_parity(ratio, 1.0, label + " achieved / bound")
    assert ratio <= 1.0, f"{label}: achieved / bound = {ratio:.3e}"
    return ratio


def held_rows(got, ref, bound, label):
    """|got - ref|_inf <= bound per configuration."""
    assert got.shape == ref.shape and not np.isnan(got).any(), label
    ratio = float((np.abs(got - ref).max(axis=1) / bound).max())
    print(f"{label}: worst err / bound = {ratio:.3e}")
    record_parity(ratio, 1.0, label + " achieved / bound")
    assert ratio <= 1.0, f"{label}: achieved / bound = {ratio:.3e}"
    return ratio


def step_bounds(ga, gb, conds, n_joints, unit, Ainf, Binf):
    """(bound of gq and gqd, bound of gtau), [B] each."""
    g1 = (0.0 if ga is None else np.abs(ga).sum(axis=1)) + (0.0 if gb is None else np.abs(gb).sum(axis=1))
    base = g1 * f32_aba_forward_factor(3 * n_joints + 1) * conds * unit
    return base * np.maximum(1.0, Ainf), base * np.maximum(1.0, Binf)


@functools.lru_cache(maxsize=None)
def model_of(case):
    from mecano_amd.engine import HipModel
    sys_, desc = make_case(case)
    return sys_, desc, HipModel(desc)


# ------------------------------------------------------------------------------------------------ 1. the integrator's transpose
@functools.lru_cache(maxsize=None)
def integrate_reference(case, dt, f32):
    sys_, desc, _ = model_of(case)
    _, qd, qdd, _ = state(sys_, B70)
    ga, gb = cotangents(B70, desc.nv)
    if f32:
        qd, qdd, ga, gb = (x.astype(np.float32).astype(np.float64) for x in (qd, qdd, ga, gb))
    return (qd, qdd, ga, gb) + svc.integrate_vjp(desc, np.float32(dt).astype(np.float64) if f32 else dt, qd, qdd, ga, gb)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("dt", [0.1, 1.0e-3])
def test_integrate_vjp_fp64_matches_checker(torch_cuda, case, layout, dt):
    _, desc, hm = model_of(case)
    qd, qdd, ga, gb, *ref, sums = integrate_reference(case, dt, False)
    got = run_integrate(torch_cuda, hm, dt, qd, qdd, ga, gb, layout)
    for g, r, s, name in zip(got, ref, sums, ("gq", "gqd", "gqdd")):
        held_entries(g, r, s, U64, f"integrate_vjp {name}")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dt", [0.1, 1.0e-3, 0.0, 1.0e-6])
def test_integrate_vjp_fp32_matches_checker_across_the_series_switch(torch_cuda, case, dt):
    """fp32 against the fp64 checker on the fp32-rounded inputs (dt included: the kernel takes (float)dt), both layouts; dt = 0 and 1e-6
    sit below so3_exp_jr's series switch and at its identity threshold."""
    torch = torch_cuda
    _, desc, hm = model_of(case)
    qd, qdd, ga, gb, *ref, sums = integrate_reference(case, dt, True)
    for layout in (AOS, SOA):
        got = run_integrate(torch, hm, dt, qd, qdd, ga, gb, layout, dtype=torch.float32)
        for g, r, s, name in zip(got, ref, sums, ("gq", "gqd", "gqdd")):
            held_entries(g, r, s, U32, f"fp32 integrate_vjp {name} layout {layout}")


# ------------------------------------------------------------------------------------------------ 2., 3. the step against A^T g', B^T g'
@functools.lru_cache(maxsize=None)
def step_reference(case, dt, with_f, f32=False):
    sys_, desc, _ = model_of(case)
    q, qd, _, tau = state(sys_, B70)
    ga, gb = cotangents(B70, desc.nv, 9)
    f = random_wrenches(np.random.default_rng(31), B70, desc.n_joints) if with_f else None
    if f32:
        q, qd, tau, ga, gb = (x.astype(np.float32).astype(np.float64) for x in (q, qd, tau, ga, gb))
        f = None if f is None else f.astype(np.float32).astype(np.float64)
    return (q, qd, tau, ga, gb, f, conds_of(desc, q)) + svc.step_vjp(desc, dt, q, qd, tau, ga, gb, GRAVITY, f)


def check_step(desc, got, ref_pack, ga, gb, conds, unit, label):
    qdd_ref, gq, gqd, gtau, _, (Ainf, Binf) = ref_pack
    close_aba(got[0], qdd_ref, None, desc.n_joints, unit, label=label + " qdd", conds=conds)
    bA, bB = step_bounds(ga, gb, conds, desc.n_joints, unit, Ainf, Binf)
    for g, r, b, name in zip(got[1:], (gq, gqd, gtau), (bA, bA, bB), ("gq", "gqd", "gtau")):
        held_rows(g, r, b, f"{label} {name}")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("dt", [0.1, 1.0e-3])
def test_step_vjp_fp64_matches_checker(torch_cuda, case, layout, dt):
    _, desc, hm = model_of(case)
    q, qd, tau, ga, gb, f, conds, *ref = step_reference(case, dt, layout == AOS)
    got = run_step(torch_cuda, hm, dt, q, qd, tau, ga, gb, f, layout)
    check_step(desc, got, ref, ga, gb, conds, U64, "step_vjp")


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("dt", [0.1, 1.0e-3])
def test_step_vjp_fp32_matches_checker(torch_cuda, case, layout, dt):
    """The same in fp32, u = 2^-24: the checker is fed the fp32-rounded inputs and the fp32-rounded dt (the kernels take (float)dt)."""
    torch = torch_cuda
    _, desc, hm = model_of(case)
    dt = float(np.float32(dt))
    q, qd, tau, ga, gb, f, conds, *ref = step_reference(case, dt, layout == AOS, True)
    got = run_step(torch, hm, dt, q, qd, tau, ga, gb, f, layout, dtype=torch.float32)
    check_step(desc, got, ref, ga, gb, conds, U32, "fp32 step_vjp")


# ------------------------------------------------------------------------------------------------ 4. one-step isolation
@pytest.mark.parametrize("case", ["humanoid30", "planar", "spherical", "onedof_tree"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_step_is_the_integrator_transpose_around_the_devices_own_aba_vjp(torch_cuda, case, layout):
    """gq = gq_int + gq_aba, gqd = gqd_int + gqd_aba, gtau = gtau_aba with (gq_int, gqd_int, w) the CHECKER's integrate_vjp at the
    device's qdd and (gq_aba, gqd_aba, gtau_aba) the device's own mh_aba_vjp_* for the w the device's kernel forms (the same launch on the
    same numbers as inside the call).  Bound per entry: 24 u abs-sum for the new kernel plus 2 u (|gq_int| + |gq_aba|) for the one
    addition and the rounding of what is added -- nothing of cond(H) in it.  gtau and qdd are the bits of mh_aba_vjp_*."""
    torch = torch_cuda
    sys_, desc, hm = model_of(case)
    dt = 0.02
    q, qd, _, tau = state(sys_, B70)
    ga, gb = cotangents(B70, desc.nv, 10)
    f = random_wrenches(np.random.default_rng(33), B70, desc.n_joints)
    qdd, gq, gqd, gtau = run_step(torch, hm, dt, q, qd, tau, ga, gb, f, layout)
    iq, iv, w_ref, (sq, sv, sw) = svc.integrate_vjp(desc, dt, qd, qdd, ga, gb)
    w_dev = run_integrate(torch, hm, dt, qd, qdd, ga, gb, layout, out=(None, None, lay(torch.empty(B70, desc.nv, dtype=torch.float64, device="cuda"), layout)))[2]
    held_entries(w_dev, w_ref, sw, U64, "isolated w")
    a = [lay(dev(torch, x), layout) for x in (q, qd, tau, w_dev, f)]
    qdd_a, gq_a, gqd_a, gtau_a = (host(t, layout) for t in hm.aba_vjp(a[0], a[1], a[2], a[3], GRAVITY, a[4], layout))
    assert np.array_equal(qdd, qdd_a) and np.array_equal(gtau, gtau_a)
    held_entries(gq, iq + gq_a, sq, U64, "isolated gq", extra=2.0 * U64 * (np.abs(iq) + np.abs(gq_a)))
    held_entries(gqd, iv + gqd_a, sv, U64, "isolated gqd", extra=2.0 * U64 * (np.abs(iv) + np.abs(gqd_a)))


# ------------------------------------------------------------------------------------------------ 5. exact cases
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_zero_step_is_exactly_the_identity(torch_cuda, dtype_name, layout):
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc, hm = model_of("humanoid30")
    q, qd, qdd, tau = (lay(dev(torch, x, dtype), layout) for x in state(sys_, B70))
    ga, gb = (lay(dev(torch, x, dtype), layout) for x in cotangents(B70, desc.nv, 11))
    f = lay(dev(torch, random_wrenches(np.random.default_rng(34), B70, desc.n_joints), dtype), layout)
    gq, gqd, gqdd = hm.integrate_vjp(0.0, qd, qdd, ga, gb, layout)
    assert bool((gq == ga).all()) and bool((gqd == gb).all()) and bool((gqdd == 0).all())
    _, gq, gqd, gtau = hm.step_vjp(0.0, q, qd, tau, ga, gb, GRAVITY, f, layout)
    assert bool((gq == ga).all()) and bool((gqd == gb).all()) and bool((gtau == 0).all())


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_a_null_cotangent_is_a_zero_cotangent(torch_cuda, layout):
    torch = torch_cuda
    sys_, desc, hm = model_of("humanoid30")
    q, qd, qdd, tau = (lay(dev(torch, x), layout) for x in state(sys_, B70))
    ga, gb = (lay(dev(torch, x), layout) for x in cotangents(B70, desc.nv, 12))
    z = torch.zeros_like(ga)
    for a, b, za, zb in ((None, gb, z, gb), (ga, None, ga, z)):
        assert all(torch.equal(x, y) for x, y in zip(hm.integrate_vjp(0.05, qd, qdd, a, b, layout), hm.integrate_vjp(0.05, qd, qdd, za, zb, layout)))
        assert all(torch.equal(x, y) for x, y in zip(hm.step_vjp(0.05, q, qd, tau, a, b, GRAVITY, None, layout),
                                                     hm.step_vjp(0.05, q, qd, tau, za, zb, GRAVITY, None, layout)))


def test_unowned_dof_indices_get_zeros_and_are_not_read(torch_cuda):
    """A custom index map with two DoF / configuration indices no joint owns: the cotangents carry NaN there; the outputs hold zeros
    there and the default map's values elsewhere (the elementwise kernel bit for bit, the step within its bound)."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, d0, h0 = model_of("onedof_tree")
    B, nv, dt = B70, d0.nv, 0.03
    q, qd, qdd, tau = state(sys_, B)
    ga, gb = cotangents(B, nv, 13)
    place = np.array([k + (k >= 3) + (k >= 7) for k in range(nv)])  # indices 3 and 8 of the wide map stay free
    free = np.setdiff1d(np.arange(nv + 2), place)
    d1 = sys_.toModelDesc()
    d1.dof_indices = place[np.asarray(d0.dof_indices)].astype(np.int32)
    d1.cfg_indices = place[np.asarray(d0.cfg_indices)].astype(np.int32)
    d1.nv = d1.nq = nv + 2
    h1 = HipModel(d1)
    wide = lambda x, fill: np.ascontiguousarray(np.insert(np.insert(x, 3, fill, axis=1), 8, fill, axis=1))
    base = run_integrate(torch, h0, dt, qd, qdd, ga, gb, AOS)
    conds, ref = conds_of(d0, q), svc.step_vjp(d0, dt, q, qd, tau, ga, gb, GRAVITY)
    bA, bB = step_bounds(ga, gb, conds, d0.n_joints, U64, *ref[5])
    for layout in (AOS, SOA):
        pois = lambda: lay(torch.full((B, nv + 2), float("nan"), dtype=torch.float64, device="cuda"), layout)
        got = run_integrate(torch, h1, dt, wide(qd, 0.25), wide(qdd, -0.5), wide(ga, np.nan), wide(gb, np.nan), layout, out=(pois(), pois(), pois()))
        for k, g in enumerate(got):
            assert not np.isnan(g).any() and not g[:, free].any() and np.array_equal(g[:, place], base[k]), f"integrate_vjp output {k}"
        got = run_step(torch, h1, dt, wide(q, 0.25), wide(qd, 0.25), wide(tau, -0.5), wide(ga, np.nan), wide(gb, np.nan), None, layout,
                       out=(pois(), pois(), pois(), pois()))
        for k, (g, r, b) in enumerate(zip(got[1:], ref[1:4], (bA, bA, bB))):
            assert not np.isnan(g).any() and not g[:, free].any(), f"step_vjp output {k}"
            held_rows(g[:, place], r, b, f"step_vjp output {k}, wide map")


@functools.lru_cache(maxsize=None)
def _scattered_reference(model, f32):
    """States and cotangents in the identity description's index space and the checker's outputs on them: once per model and precision,
    shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if f32 else np.float64
    dt = float(np_dt(0.05))
    q, qd, qdd, tau = DistinctRows(sys_, 16, seed=55).rows(np.arange(B70), np_dt)
    ga, gb = (x.astype(np_dt).astype(np.float64) for x in cotangents(B70, d0.nv, 56))
    f = random_wrenches(np.random.default_rng(57), B70, d0.n_joints).astype(np_dt).astype(np.float64)
    conds = conds_of(d0, q)
    assert conds.max() < 1.0e8
    return (dt, q, qd, qdd, tau, ga, gb, f, conds, svc.integrate_vjp(d0, dt, qd, qdd, ga, gb), svc.step_vjp(d0, dt, q, qd, tau, ga, gb, GRAVITY, f))


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """integrate_vjp and step_vjp on a description whose maps send every DoF and every configuration entry somewhere else (with holes:
    two indices of each space owned by no joint, holding 7.0 in every input, the cotangents included), against the checker on the
    IDENTITY description.  The cotangents go in and every gradient comes back through the DoF map, under this file's bounds (held_entries
    for the integrator's transpose, check_step's for the step); the gradients at unowned indices are exact zeros, the guard rows stay
    poisoned; each gradient asked for alone (the other outputs NULL) meets the same bound; read without moving them back the outputs
    miss the reference by more than 1e-3."""
    torch = torch_cuda
    f32 = dtype_name == "float32"
    dtype, unit = getattr(torch, dtype_name), (U32 if f32 else U64)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, n = hp.scattered_model(d, model), B70, d.nv, d0.n_joints
    dt, q, qd, qdd, tau, ga, gb, f, conds, ref_i, ref_s = _scattered_reference(model, f32)
    tq = lay(dev(torch, hp.to_q(q, pq, d.nq), dtype), layout)
    tqd, tqdd, ttau, tga, tgb = (lay(dev(torch, hp.to_v(x, pv, nv), dtype), layout) for x in (qd, qdd, tau, ga, gb))
    tf = lay(dev(torch, f, dtype), layout)
    is_soa = layout == SOA

    def run(issue, places, want):
        outs, guards = hp.poisoned_set(torch, B, [(nv,)] * places, dtype, is_soa)
        outs = [o if k in want else None for k, o in enumerate(outs)]
        issue(tuple(outs))
        torch.cuda.synchronize()
        hp.guards_intact([g for k, g in enumerate(guards) if k in want])
        return [None if o is None else hp.from_v(hp.rows_of(o, B, (nv,), is_soa), pv) + (hp.rows_of(o, B, (nv,), is_soa),) for o in outs]

    integrate = lambda out: hm.integrate_vjp(dt, tqd, tqdd, tga, tgb, layout, out=out)
    step = lambda out: hm.step_vjp(dt, tq, tqd, ttau, tga, tgb, GRAVITY, tf, layout, out=out)
    *ref, sums = ref_i
    got = run(integrate, 3, (0, 1, 2))
    for k, (r, s, name) in enumerate(zip(ref, sums, ("gq", "gqd", "gqdd"))):
        for (back, free, raw), what in ((got[k], ""), (run(integrate, 3, (k,))[k], " alone")):
            assert not free.any(), name  # exact zeros, and written
            held_entries(back, r, s, unit, f"scattered integrate_vjp {name}{what}")
        hp.assert_misses(hp.keep_order(got[k][2], pv), r, "integrate_vjp " + name)
    qdd_ref, gq, gqd, gtau, _, (Ainf, Binf) = ref_s
    bA, bB = step_bounds(ga, gb, conds, n, unit, Ainf, Binf)
    got = run(step, 4, (0, 1, 2, 3))
    close_aba(got[0][0], qdd_ref, None, n, unit, label="scattered step_vjp qdd", conds=conds)
    for k, (r, b, name) in enumerate(zip((gq, gqd, gtau), (bA, bA, bB), ("gq", "gqd", "gtau")), start=1):
        for (back, free, raw), what in ((got[k], ""), (run(step, 4, (k,))[k], " alone")):
            assert not free.any(), name
            held_rows(back, r, b, f"scattered step_vjp {name}{what}")
        hp.assert_misses(hp.keep_order(got[k][2], pv), r, "step_vjp " + name)


@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_chart_maps_on_scattered_index_maps(torch_cuda, model, holes):
    """chart_cotangent and chart_pullback (torch operations on the description's index maps, here on device tensors) on scattered maps
    against the tangent map T of q (+) dq built from its definition on the IDENTITY description (tests/test_step_vjp_cpu.py, whose bound
    this is: 1e-14 max(1, |ref|_inf)): the cotangent is T^T g_raw; at unit quaternions the pull-back is T g with the quaternion rows
    taken four times ((2 / |Q|) Q o (g, 0) against the column Q o (e_k, 0) / 2).  q and g_raw live in the configuration space, g in the
    DoF space; unowned entries hold 7.0 on the way in and exact zeros on the way out; read without moving them back both miss the
    reference by more than 1e-3."""
    from test_step_vjp_cpu import tangent_map
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B = hp.scattered_model(d, model), B70
    q = DistinctRows(sys_, 16, seed=58).rows(np.arange(B))[0]
    rng = np.random.default_rng(59)
    g_raw, g = rng.uniform(-1.0, 1.0, (B, d0.nq)), rng.uniform(-1.0, 1.0, (B, d0.nv))
    T = np.stack([tangent_map(d0, q[b]) for b in range(B)])
    quat_rows = np.array(sorted(c for rows in mha.chart_maps(d0)["quat_q"] for c in rows), dtype=int)
    assert len(quat_rows) and np.abs(np.linalg.norm(q[:, quat_rows[:4]], axis=1) - 1.0).max() < 1e-12
    T4 = T.copy()
    T4[:, quat_rows, :] *= 4.0
    ref_cot, ref_pull = np.einsum("bqv,bq->bv", T, g_raw), np.einsum("bqv,bv->bq", T4, g)
    tq = dev(torch, hp.to_q(q, pq, d.nq))
    cot = hm.chart_cotangent(tq, dev(torch, hp.to_q(g_raw, pq, d.nq))).cpu().numpy()
    pull = hm.chart_pullback(tq, dev(torch, hp.to_v(g, pv, d.nv))).cpu().numpy()
    for raw, perm, ref, name in ((cot, pv, ref_cot, "chart_cotangent"), (pull, pq, ref_pull, "chart_pullback")):
        back, free = hp.from_v(raw, perm)
        assert not np.isnan(raw).any() and not free.any(), name
        err, bound = float(np.abs(back - ref).max()), 1.0e-14 * max(1.0, float(np.abs(ref).max()))
        record_parity(err, bound, f"scattered {name}")
        assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
        hp.assert_misses(hp.keep_order(raw, perm), ref, name)


# ------------------------------------------------------------------------------------------------ 6. cover of batches
@functools.lru_cache(maxsize=None)
def cover_reference(case, B, grid, dt, group=64, step_rows=None):
    """The inputs' generators and the checker's results on the rows the cover takes, computed once per (case, B)."""
    sys_, desc, _ = model_of(case)
    rows = DistinctRows(sys_, 256, seed=29)
    idx = group_cover(B, grid, group)
    ga64, gb64 = cotangents(64, desc.nv, 13)
    f64 = random_wrenches(np.random.default_rng(24), 64, desc.n_joints)
    q, qd, qdd, tau = rows.rows(idx)
    ref_i = svc.integrate_vjp(desc, dt, qd, qdd, ga64[idx % 64], gb64[idx % 64])
    sidx = idx if step_rows is None else np.asarray(step_rows)
    q, qd, _, tau = rows.rows(sidx)
    ref_s = svc.step_vjp(desc, dt, q, qd, tau, ga64[sidx % 64], gb64[sidx % 64], GRAVITY, f64[sidx % 64])
    return rows, idx, sidx, ga64, gb64, f64, ref_i, ref_s, conds_of(desc, q)


def cover_case(torch, case, B, grid, layout, which, skip=None, dt=0.02, group=64, step_rows=None):
    """B distinct rows, poisoned outputs with a guard row behind them, every row group checked; `skip`: index (or tuple of indices) of
    the outputs passed as NULL.  which: "integrate" or "step"."""
    skips = skip if isinstance(skip, tuple) else (skip,)
    _, desc, hm = model_of(case)
    rows, idx, sidx, ga64, gb64, f64, ref_i, ref_s, conds = cover_reference(case, B, grid, dt, group, step_rows)
    nv = desc.nv
    q, qd, qdd, tau = rows.device(torch, B)
    period = torch.arange(B, device="cuda") % 64
    ga, gb, f = (dev(torch, x)[period].contiguous() for x in (ga64, gb64, f64))
    outs, guards = [], []
    for k in range(3 if which == "integrate" else 4):
        o, g = (None, None) if k in skips else (poisoned(torch, B, (nv,), torch.float64) if layout == AOS else poisoned(torch, nv, (B,), torch.float64))
        outs.append(o), guards.append(g)
    L = lambda t: lay(t, layout)
    if which == "integrate":
        hm.integrate_vjp(dt, L(qd), L(qdd), L(ga), L(gb), layout, out=tuple(outs))
        take, refs, sums = idx, ref_i[:3], ref_i[3]
    else:
        hm.step_vjp(dt, L(q), L(qd), L(tau), L(ga), L(gb), GRAVITY, L(f), layout, out=tuple(outs))
        take, refs = sidx, ref_s[:4]
        bA, bB = step_bounds(ga64[sidx % 64], gb64[sidx % 64], conds, desc.n_joints, U64, *ref_s[5])
    torch.cuda.synchronize()
    at = torch.as_tensor(take, device="cuda")
    for k, (o, g, r) in enumerate(zip(outs, guards, refs)):
        if o is None:
            continue
        assert torch.isnan(g).all(), f"output {k}: wrote past the last row"
        assert not torch.isnan(o).any(), f"output {k}: rows left unwritten (NaN)"
        got = (o if layout == AOS else o.t())[at].cpu().numpy()
        if which == "integrate":
            held_entries(got, r, sums[k], U64, f"cover integrate_vjp output {k}")
        elif k == 0:
            close_aba(got, r, None, desc.n_joints, U64, label="cover qdd", conds=conds)
        else:
            held_rows(got, r, bB if k == 3 else bA, f"cover step_vjp output {k}")


@pytest.mark.parametrize("skip", [None, 0, 1, 2])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_integrate_vjp_each_output_null_in_turn(torch_cuda, skip, layout):
    cover_case(torch_cuda, "humanoid30", 64 * 5 + 3, None, layout, "integrate", skip)


@pytest.mark.parametrize("skip", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_step_vjp_each_output_null_in_turn(torch_cuda, skip, layout):
    cover_case(torch_cuda, "humanoid30", 64 * 5 + 3, None, layout, "step", skip)


@pytest.mark.parametrize("skip", [(0, 1, 2), (1, 2), (0, 3)])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_step_vjp_outputs_null_together(torch_cuda, skip, layout):
    """gtau alone (the first forward-dynamics launch still runs: the cotangent of qdd needs qdd wherever dt != 0), qdd and gtau without
    gq and gqd (no adjoint launch), and gq and gqd with qdd and gtau both in the context's scratch behind w."""
    cover_case(torch_cuda, "humanoid30", 64 * 5 + 3, None, layout, "step", skip)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case,B", [("arm7", 1), ("arm7", 65), ("humanoid30", 197)])
def test_step_vjp_outputs_null_together_leave_the_others_bit_for_bit(torch_cuda, case, B, layout, dtype_name):
    """Small batches (one lane, a ragged second wave, several waves per group), both precisions: gtau alone, qdd and gtau, gq and gqd
    (qdd and gtau in the context's scratch behind w), qdd without gtau and gtau without qdd -- what is asked for has the bits of the
    call that asks for everything, which the tests above hold to the checker."""
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc, hm = model_of(case)
    q, qd, _, tau = state(sys_, B)
    ga, gb = cotangents(B, desc.nv)
    f = random_wrenches(np.random.default_rng(24), B, desc.n_joints)
    put = lambda x: lay(dev(torch, x.reshape(B, -1), dtype), layout)
    Q, QD, TAU, GA, GB, F = (put(x) for x in (q, qd, tau, ga, gb, f))
    full = hm.step_vjp(0.02, Q, QD, TAU, GA, GB, GRAVITY, F, layout)
    assert all(torch.isfinite(t).all() for t in full)
    for keep in ((3,), (0, 3), (1, 2), (0, 1, 2), (1, 2, 3)):  # of (qdd, gq, gqd, gtau)
        outs = tuple(torch.full_like(t, float("nan")) if k in keep else None for k, t in enumerate(full))
        res = hm.step_vjp(0.02, Q, QD, TAU, GA, GB, GRAVITY, F, layout, out=outs)
        torch.cuda.synchronize()
        assert all((r is None) if k not in keep else torch.equal(r, full[k]) for k, r in enumerate(res)), keep


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the lanes the elementwise kernel's planned grid holds (8 workgroups of 256 lanes, or of a 256-row tile, per CU),
    plus a full and a ragged group: every lane loops.  mh_integrate_vjp_* on a row of every group of 256 and every row of the first group
    of each turn of the loop; the step on the first and last groups (its other launches have their own cover tests)."""
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    # the grid integrate_vjp_launch plans (mh_api.hip): at most 8 workgroups per CU, 256 lanes (SoA) or a tile of up to 256 rows (AoS,
    # reached from B = 1024 rows per CU on) each -- a change of that plan has to be followed here, or the batch stops filling the device
    lanes = 8 * cus * 256
    B = 2 * lanes + 64 + 37
    step_rows = tuple(np.r_[0:64, lanes:lanes + 4, 2 * lanes:B].tolist())
    cover_case(torch, "arm7", B, 8 * cus, layout, "integrate", group=256, step_rows=step_rows)
    cover_case(torch, "arm7", B, 8 * cus, layout, "step", group=256, step_rows=step_rows)


# ------------------------------------------------------------------------------------------------ 7. plumbing
def graph_edges(graph):
    """(edges, number of nodes) of a captured graph kept by torch (``keep_graph=True``), from the HIP runtime itself."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    g, n, nodes = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(n)) == 0 and hip.hipGraphGetNodes(g, None, ctypes.byref(nodes)) == 0
    a, b = (ctypes.c_void_p * n.value)(), (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetEdges(g, a, b, ctypes.byref(n)) == 0
    return list(zip(a, b)), nodes.value


def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() and a first call both calls are captured
    into a graph (they allocate nothing), the captured launches form one chain, and the replay gives the bits of the direct call, also on
    changed inputs."""
    torch = torch_cuda
    sys_, desc, hm = model_of("humanoid30")
    B, dt = 1000, 0.01
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    ga, gb = (dev(torch, x) for x in cotangents(B, desc.nv, 14))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    ref_i = hm.integrate_vjp(dt, qd, qdd, ga, gb)
    ref_s = hm.step_vjp(dt, q, qd, tau, ga, gb, GRAVITY, f)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    out_i = tuple(torch.empty_like(t) for t in ref_i)
    out_s = tuple(torch.empty_like(t) for t in ref_s[1:3])

    def issue():
        view.integrate_vjp(dt, qd, qdd, ga, gb, out=out_i)
        view.step_vjp(dt, q, qd, tau, ga, gb, GRAVITY, f, out=(None, out_s[0], out_s[1], None))  # qdd, w and H^-1 w in the context's scratch

    same = lambda ri, rs: all(torch.equal(a, b) for a, b in zip(out_i, ri)) and all(torch.equal(a, b) for a, b in zip(out_s, rs[1:3]))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        issue()
        view.check(s.cuda_stream)
        assert same(ref_i, ref_s)
        for t in out_i + out_s:
            t.zero_()
        torch.cuda.synchronize()
        graph, kept = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, stream=s):
            issue()
        with torch.cuda.graph(kept, stream=s):  # the same capture once more, kept as a graph to look at its edges
            issue()
    torch.cuda.synchronize()
    assert not any(t.any() for t in out_i + out_s)  # captured, not executed
    edges, nodes = graph_edges(kept)
    assert nodes >= 6  # the elementwise launch; then forward dynamics, the elementwise launch, a memset, forward dynamics, the sweep
    heads, tails = [a for a, _ in edges], [b for _, b in edges]
    assert len(edges) == nodes - 1 and len(set(heads)) == len(heads) and len(set(tails)) == len(tails), \
        f"the captured launches do not form one chain: {nodes} nodes, edges {edges}"
    del kept
    graph.replay()
    torch.cuda.synchronize()
    assert same(ref_i, ref_s)
    q2, qd2 = dev(torch, state(sys_, B, seed=6)[0]), dev(torch, state(sys_, B, seed=6)[1])
    ga2 = dev(torch, cotangents(B, desc.nv, 15)[0])
    ref_i2 = hm.integrate_vjp(dt, qd2, qdd, ga2, gb)
    ref_s2 = hm.step_vjp(dt, q2, qd2, tau, ga2, gb, GRAVITY, f)
    q.copy_(q2), qd.copy_(qd2), ga.copy_(ga2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same(ref_i2, ref_s2)
    view.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_poisoned_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n, dt = HipModel(desc), 10, desc.nv, desc.n_joints, 0.01
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    ga, gb = (dev(torch, x) for x in cotangents(B, nv, 16))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    nan = lambda: torch.full((B, nv), float("nan"), dtype=torch.float64, device="cuda")
    icall = lambda out, dt_=dt, a=ga, b=gb: hm.integrate_vjp(dt_, qd, qdd, a, b, out=out)
    scall = lambda out, dt_=dt, a=ga, b=gb, fe=None: hm.step_vjp(dt_, q, qd, tau, a, b, GRAVITY, fe, out=out)
    for call, n_out in ((icall, 3), (scall, 4)):
        outs = [nan() for _ in range(n_out)]

        def refused(**kw):
            with pytest.raises(_lib.MecanoHipError):
                call(tuple(outs), **kw)
            torch.cuda.synchronize()
            assert all(torch.isnan(o).all() for o in outs)

        refused(a=None, b=None)                                      # both cotangents NULL
        for bad in (float("nan"), float("inf"), -float("inf")):      # a step that is not finite
            refused(dt_=bad)
        for bad in (z(B, nv + 1), z(nv, B), z(B + 1, nv)):           # wrong shapes
            refused(a=bad)
            refused(b=bad)
        with pytest.raises(_lib.MecanoHipError):                     # all gradient outputs NULL (qdd alone is not one)
            call((None,) * 3 if n_out == 3 else (outs[0], None, None, None))
        with pytest.raises(_lib.MecanoHipError):
            call(tuple(outs[:-1]))
        check_bad_outputs(torch, [(B, nv)] * n_out, call)
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(B, n, 5), z(n * 6, B)):
        with pytest.raises(_lib.MecanoHipError):
            scall(None, fe=bad_f)
    with pytest.raises(_lib.MecanoHipError):
        hm.integrate_vjp(dt, qd, z(B + 1, nv), ga, gb)
    with pytest.raises(_lib.MecanoHipError):
        hm.step_vjp(dt, q, z(B, nv + 1), tau, ga, gb, GRAVITY)
    # every forbidden overlap: an output on an input (q has nq = nv here), two outputs on each other -- nothing is written
    for call, inputs, n_out in ((icall, (qd, qdd, ga, gb), 3), (scall, (q, qd, tau, ga, gb), 4)):
        before = [t.clone() for t in inputs]
        for k in range(n_out):
            for t in inputs:
                outs = [nan() for _ in range(n_out)]
                outs[k] = t
                with pytest.raises(_lib.MecanoHipError):
                    call(tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for j, o in enumerate(outs) if j != k)
            for j in range(k):
                outs = [nan() for _ in range(n_out)]
                outs[k] = outs[j]
                with pytest.raises(_lib.MecanoHipError):
                    call(tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for o in outs)
        assert all(torch.equal(a, b) for a, b in zip(inputs, before))
    modes = [0] * n
    modes[2] = 1
    hm.set_joint_source_modes(modes)
    outs = [nan() for _ in range(4)]
    with pytest.raises(_lib.MecanoHipError):  # source joints: the step call only
        scall(tuple(outs))
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    free = hm.integrate_vjp(dt, qd, qdd, ga, gb)
    hm.set_joint_source_modes(None)
    assert all(torch.equal(a, b) for a, b in zip(free, hm.integrate_vjp(dt, qd, qdd, ga, gb)))
    # B = 0: MH_OK through the bare C-ABI, nothing touched
    import ctypes
    lib, p = _lib.load(), lambda t: t.data_ptr()
    opts = hm._options(0, stream=torch.cuda.current_stream().cuda_stream)
    g3, o0 = (ctypes.c_double * 3)(*GRAVITY), nan()
    assert lib.mh_integrate_vjp_f64(hm._h, 0, dt, None, None, p(ga), None, ctypes.byref(opts), p(o0), None, None) == 0
    assert lib.mh_aba_integrate_vjp_f64(hm._h, 0, dt, None, None, None, g3, None, p(ga), None, ctypes.byref(opts), None, p(o0), None, None) == 0
    # the library's own refusals, which the Python layer never lets through: both cotangents NULL, every gradient output NULL (qdd_out
    # alone is no gradient) -- MH_ERR_INVALID_ARGUMENT, nothing written
    o1, pv = nan(), lambda *ts: [p(t) for t in ts]
    by = ctypes.byref(opts)
    for fn in (lib.mh_integrate_vjp_f64, lib.mh_integrate_vjp_f32):
        assert fn(hm._h, B, dt, *pv(qd, qdd), None, None, by, *pv(o0, o1), None) == 1
        assert fn(hm._h, B, dt, *pv(qd, qdd, ga, gb), by, None, None, None) == 1
        assert lib.mh_last_error()
    for fn in (lib.mh_aba_integrate_vjp_f64, lib.mh_aba_integrate_vjp_f32):
        assert fn(hm._h, B, dt, *pv(q, qd, tau), g3, None, None, None, by, None, *pv(o0, o1), None) == 1
        assert fn(hm._h, B, dt, *pv(q, qd, tau), g3, None, *pv(ga, gb), by, p(o0), None, None, None) == 1
        assert fn(hm._h, B, dt, *pv(q, qd, tau), None, None, *pv(ga, gb), by, None, *pv(o0, o1), None) == 1  # no gravity, no root acceleration
        assert lib.mh_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(o0).all() and torch.isnan(o1).all()


# ------------------------------------------------------------------------------------------------ 9. autograd
def manual_backward(torch, mha, hm, desc, dt, q, qd, tau, q_next, g_raw_next, g_qd_next, f=None):
    """chart_cotangent -> ONE step_vjp -> chart_pullback + the radial term: what autograd.step's backward pass is."""
    gth = hm.chart_cotangent(q_next, g_raw_next)
    _, gq, gqd, gtau = hm.step_vjp(dt, q, qd, tau, gth, g_qd_next.contiguous(), GRAVITY, f, out=(None,) + tuple(torch.empty_like(qd) for _ in range(3)))
    return hm.chart_pullback(q, gq) + mha.radial_passthrough(desc, q, q_next, g_raw_next), gqd, gtau


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_autograd_step_is_the_vjp_call_between_the_two_chart_maps(torch_cuda, dtype_name):
    """autograd.step's gradients are chart_cotangent -> step_vjp -> chart_pullback + the radial term bit for bit (fp64: the forward is
    HipModel.step, fp32: aba then integrate); autograd.integrate likewise with integrate_vjp; an input that does not require a gradient
    yields None; a second backward raises."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc, hm = model_of("humanoid30")
    B, dt = B70, 0.01
    qh, qdh, qddh, tauh = state(sys_, B)
    cq, cv = dev(torch, np.random.default_rng(3).uniform(-1.0, 1.0, (B, desc.nq)), dtype), dev(torch, cotangents(B, desc.nv, 17)[0], dtype)
    f = dev(torch, random_wrenches(np.random.default_rng(27), B, desc.n_joints), dtype)
    q, qd, tau = (dev(torch, x, dtype).requires_grad_() for x in (qh, qdh, tauh))
    qn, vn = mha.step(hm, dt, q, qd, tau, GRAVITY, f)
    if dtype == torch.float64:
        ref_n = hm.step(dt, q.detach(), qd.detach(), tau.detach(), GRAVITY, f)[:2]
    else:
        ref_n = hm.integrate(dt, q.detach(), qd.detach(), hm.aba(q.detach(), qd.detach(), tau.detach(), GRAVITY, f))[:2]
    assert torch.equal(qn, ref_n[0]) and torch.equal(vn, ref_n[1])
    got = torch.autograd.grad((cq * qn).sum() + (cv * vn).sum(), (q, qd, tau))
    want = manual_backward(torch, mha, hm, desc, dt, q.detach(), qd.detach(), tau.detach(), qn.detach(), cq, cv, f)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # the integrator alone
    q, qd, qdd = (dev(torch, x, dtype).requires_grad_() for x in (qh, qdh, qddh))
    qn, vn = mha.integrate(hm, dt, q, qd, qdd)
    got = torch.autograd.grad((cq * qn).sum() + (cv * vn).sum(), (q, qd, qdd))
    gq, gqd, gqdd = hm.integrate_vjp(dt, qd.detach(), qdd.detach(), hm.chart_cotangent(qn.detach(), cq), cv)
    want = (hm.chart_pullback(q.detach(), gq) + mha.radial_passthrough(desc, q.detach(), qn.detach(), cq), gqd, gqdd)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # only qd asks
    q, qd, tau = dev(torch, qh, dtype), dev(torch, qdh, dtype).requires_grad_(), dev(torch, tauh, dtype)
    qn, vn = mha.step(hm, dt, q, qd, tau, GRAVITY, f)
    (gqd,) = torch.autograd.grad((cq * qn).sum() + (cv * vn).sum(), (qd,), create_graph=True)
    assert torch.equal(gqd, manual_backward(torch, mha, hm, desc, dt, q, qd.detach(), tau, qn.detach(), cq, cv, f)[1])
    with pytest.raises(RuntimeError):
        gqd.sum().backward()


def test_autograd_rollout_is_the_manual_reverse_loop(torch_cuda):
    """Three steps of humanoid30, B = 8, through autograd against the same calls in a hand-written reverse loop, bit for bit."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, desc, hm = model_of("humanoid30")
    B, dt, steps = 8, 0.005, 3
    qh, qdh, _, tauh = state(sys_, B)
    taus = [dev(torch, tauh * (1.0 + 0.1 * k)).requires_grad_() for k in range(steps)]
    q0, qd0 = dev(torch, qh).requires_grad_(), dev(torch, qdh).requires_grad_()
    cq, cv = dev(torch, np.random.default_rng(5).uniform(-1.0, 1.0, (B, desc.nq))), dev(torch, cotangents(B, desc.nv, 18)[0])
    q, qd, traj = q0, qd0, []
    for k in range(steps):
        traj.append((q.detach(), qd.detach()))
        q, qd = mha.step(hm, dt, q, qd, taus[k], GRAVITY, None)
    got = torch.autograd.grad((cq * q).sum() + (cv * qd).sum(), [q0, qd0] + taus)
    g_q, g_qd, g_tau, q_next = cq, cv, [None] * steps, q.detach()
    for k in reversed(range(steps)):
        qk, qdk = traj[k]
        g_q, g_qd, g_tau[k] = manual_backward(torch, mha, hm, desc, dt, qk, qdk, taus[k].detach(), q_next, g_q, g_qd)
        q_next = qk
    assert all(torch.equal(a, b) for a, b in zip(got, [g_q, g_qd] + g_tau))


def test_autograd_step_against_central_differences_of_the_step(torch_cuda):
    """One fp64 step of humanoid30 with a non-unit base quaternion, B = 4, no wrenches: the gradient of c_q . q_next_raw + c_v . qd_next
    with respect to RAW q, qd and tau against central differences (h = 1e-5) of HipModel.step on the quaternion entries and three other
    components of each input.  Bound: 2e-5 cond_inf(H) |c|_1 max(1, |gradient|_inf), the form of tests/test_step_derivatives_cpu.py."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, desc, hm = model_of("humanoid30")
    B, dt, h = 4, 0.01, 1.0e-5
    qh, qdh, _, tauh = state(sys_, B)
    quat = mha.chart_maps(desc)["quat_q"][0]
    qh[:, quat] *= np.array([1.0, 0.7, 1.4, 1.9])[:, None]
    rng = np.random.default_rng(6)
    cqh, cvh = rng.uniform(-1.0, 1.0, (B, desc.nq)), rng.uniform(-1.0, 1.0, (B, desc.nv))
    cq, cv = dev(torch, cqh), dev(torch, cvh)
    q, qd, tau = (dev(torch, x).requires_grad_() for x in (qh, qdh, tauh))
    qn, vn = mha.step(hm, dt, q, qd, tau, GRAVITY, None)
    grads = [g.cpu().numpy() for g in torch.autograd.grad((cq * qn).sum() + (cv * vn).sum(), (q, qd, tau))]

    def loss(x):
        a, b, _ = hm.step(dt, *(dev(torch, t) for t in x), GRAVITY, None)
        return (cq * a).sum(1).cpu().numpy() + (cv * b).sum(1).cpu().numpy()

    conds = conds_of(desc, qh)
    c1 = np.abs(cqh).sum(axis=1) + np.abs(cvh).sum(axis=1)
    others = [k for k in range(desc.nq) if k not in quat]
    picks = ([*quat, others[0], others[len(others) // 2], others[-1]], [0, desc.nv // 2, desc.nv - 1], [0, desc.nv // 2, desc.nv - 1])
    base = [qh, qdh, tauh]
    for which, (g, cols) in enumerate(zip(grads, picks)):
        bound = 2.0e-5 * conds * c1 * np.maximum(1.0, np.abs(g).max(axis=1))
        for k in cols:
            e = np.zeros_like(base[which])
            e[:, k] = h
            plus, minus = [x.copy() for x in base], [x.copy() for x in base]
            plus[which] += e
            minus[which] -= e
            fd = (loss(plus) - loss(minus)) / (2.0 * h)
            ratio = float((np.abs(g[:, k] - fd) / bound).max())
            print(f"input {which} component {k}: |autograd - central difference| / bound = {ratio:.3e}")
            record_parity(ratio, 1.0, f"input {which} component {k} achieved / bound")
            assert ratio <= 1.0, f"input {which} component {k}: achieved / bound = {ratio:.3e}"
