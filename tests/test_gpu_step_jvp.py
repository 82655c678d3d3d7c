"""mh_integrate_jvp_* / mh_aba_integrate_jvp_* on the device against the CPU checker (tests/dynamics_jvp_check.py: the matrices of
tests/step_derivatives_check.py applied to the directions, pinned by tests/test_dynamics_jvp_cpu.py).  The reference is the checker only,
never the code under test.

Bounds.  mh_integrate_jvp_*: per ENTRY 24 u x the sum of the absolute terms of that entry (|G|_abs |d|), as held_entries of
tests/test_gpu_step_vjp.py takes it for the transposed blocks; an entry with a zero bound is exactly zero.  mh_aba_integrate_jvp_*: per
configuration (|dx|_1 max(1, |A_ref|_inf) + |dtau|_1 max(1, |B_ref|_inf)) f32_aba_forward_factor(3 n + 1) cond_inf(H) u on dq_next and
dqd_next, the bound of tests/test_gpu_dynamics_jvp.py on dqdd, helpers.close_aba on qdd.  fp32: u = 2^-24, the checker fed the
fp32-rounded inputs.  Every check records achieved / bound (helpers.record_parity)."""
import functools

import numpy as np
import pytest

import dynamics_jvp_check as jc
import helpers as hp
from helpers import DistinctRows, check_bad_outputs, close_aba, f32_aba_forward_factor, group_cover, poisoned
from test_gpu_dynamics_jvp import aba_bound, directions, l1
from test_gpu_step_vjp import AOS, B70, SOA, U32, U64, conds_of, cotangents, dev, held_entries, held_rows, host, lay, model_of, state
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def run_integrate(torch, hm, dt, qd, qdd, ds, layout, dtype=None, **kw):
    """hm.integrate_jvp on host arrays: (dq_next, dqd_next) as AoS-shaped fp64 arrays."""
    a = [lay(dev(torch, x, dtype), layout) for x in (qd, qdd) + tuple(ds)]
    out = hm.integrate_jvp(dt, *a, layout, **kw)
    torch.cuda.synchronize()
    return tuple(host(t, layout) for t in out)


def run_step(torch, hm, dt, q, qd, tau, ds, f, layout, dtype=None, **kw):
    """hm.step_jvp on host arrays: (qdd, dqdd, dq_next, dqd_next) as AoS-shaped fp64 arrays."""
    a = [lay(dev(torch, x, dtype), layout) for x in (q, qd, tau) + tuple(ds) + (f,)]
    out = hm.step_jvp(dt, *a[:6], GRAVITY, a[6], layout, **kw)
    torch.cuda.synchronize()
    return tuple(host(t, layout) for t in out)


def step_bound(ds, conds, n_joints, unit, Ainf, Binf):
    B = len(conds)
    return ((l1(ds[0], B) + l1(ds[1], B)) * np.maximum(1.0, Ainf) + l1(ds[2], B) * np.maximum(1.0, Binf)) * f32_aba_forward_factor(3 * n_joints + 1) * conds * unit


# ------------------------------------------------------------------------------------------------ 1. the integrator's tangent map
@functools.lru_cache(maxsize=None)
def integrate_reference(case, dt, f32):
    sys_, desc, _ = model_of(case)
    _, qd, qdd, _ = state(sys_, B70)
    ds = directions(B70, desc.nv)
    if f32:
        qd, qdd = (x.astype(np.float32).astype(np.float64) for x in (qd, qdd))
        ds = tuple(d.astype(np.float32).astype(np.float64) for d in ds)
    return (qd, qdd, ds) + jc.integrate_jvp(desc, np.float32(dt).astype(np.float64) if f32 else dt, qd, qdd, *ds)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("dt", [0.1, 1.0e-3])
def test_integrate_jvp_fp64_matches_checker(torch_cuda, case, layout, dt):
    _, desc, hm = model_of(case)
    qd, qdd, ds, *ref, sums = integrate_reference(case, dt, False)
    got = run_integrate(torch_cuda, hm, dt, qd, qdd, ds, layout)
    for g, r, s, name in zip(got, ref, sums, ("dq_next", "dqd_next")):
        held_entries(g, r, s, U64, f"integrate_jvp {name}")


@pytest.mark.parametrize("case", ["arm7", "humanoid30", "planar", "spherical"])
@pytest.mark.parametrize("dt", [0.1, 1.0e-3, 0.0, 1.0e-6])
def test_integrate_jvp_fp32_matches_checker_across_the_series_switch(torch_cuda, case, dt):
    """fp32 against the fp64 checker on the fp32-rounded inputs (dt included: the kernel takes (float)dt), both layouts; dt = 0 and 1e-6
    sit below so3_exp_jr's series switch and at its identity threshold."""
    torch = torch_cuda
    _, desc, hm = model_of(case)
    qd, qdd, ds, *ref, sums = integrate_reference(case, dt, True)
    for layout in (AOS, SOA):
        got = run_integrate(torch, hm, dt, qd, qdd, ds, layout, dtype=torch.float32)
        for g, r, s, name in zip(got, ref, sums, ("dq_next", "dqd_next")):
            held_entries(g, r, s, U32, f"fp32 integrate_jvp {name} layout {layout}")


# ------------------------------------------------------------------------------------------------ 2. the step against A dx + B dtau
@functools.lru_cache(maxsize=None)
def step_reference(case, dt, with_f, f32=False):
    sys_, desc, _ = model_of(case)
    q, qd, _, tau = state(sys_, B70)
    ds = directions(B70, desc.nv, 9)
    f = random_wrenches(np.random.default_rng(31), B70, desc.n_joints) if with_f else None
    if f32:
        q, qd, tau = (x.astype(np.float32).astype(np.float64) for x in (q, qd, tau))
        ds = tuple(d.astype(np.float32).astype(np.float64) for d in ds)
        f = None if f is None else f.astype(np.float32).astype(np.float64)
    return (q, qd, tau, ds, f, conds_of(desc, q)) + jc.step_jvp(desc, dt, q, qd, tau, *ds, GRAVITY, f)


def check_step(desc, got, ref_pack, ds, conds, unit, label):
    qdd_ref, dqdd, dqn, dqdn, _, (Ainf, Binf), scales = ref_pack
    close_aba(got[0], qdd_ref, None, desc.n_joints, unit, label=label + " qdd", conds=conds)
    held_rows(got[1], dqdd, aba_bound(ds, scales, conds, desc.n_joints, unit), f"{label} dqdd")
    b = step_bound(ds, conds, desc.n_joints, unit, Ainf, Binf)
    for g, r, name in zip(got[2:], (dqn, dqdn), ("dq_next", "dqd_next")):
        held_rows(g, r, b, f"{label} {name}")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("with_f", [False, True])
def test_step_jvp_fp64_matches_checker(torch_cuda, case, layout, with_f):
    dt = 0.1 if with_f else 1.0e-3
    _, desc, hm = model_of(case)
    q, qd, tau, ds, f, conds, *ref = step_reference(case, dt, with_f)
    got = run_step(torch_cuda, hm, dt, q, qd, tau, ds, f, layout)
    check_step(desc, got, ref, ds, conds, U64, "step_jvp")


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_step_jvp_fp32_matches_checker(torch_cuda, case, layout):
    """The same in fp32, u = 2^-24: the checker is fed the fp32-rounded inputs and the fp32-rounded dt (the kernels take (float)dt)."""
    torch = torch_cuda
    _, desc, hm = model_of(case)
    dt = float(np.float32(0.01))
    q, qd, tau, ds, f, conds, *ref = step_reference(case, dt, True, True)
    got = run_step(torch, hm, dt, q, qd, tau, ds, f, layout, dtype=torch.float32)
    check_step(desc, got, ref, ds, conds, U32, "fp32 step_jvp")


# ------------------------------------------------------------------------------------------------ 3. device against device
@pytest.mark.parametrize("case", ["humanoid30", "planar", "spherical"])
def test_step_is_aba_jvp_then_integrate_jvp_and_contracts_the_device_matrices(torch_cuda, case):
    """step_jvp has the bits of aba_jvp followed by integrate_jvp; (dq_next, dqd_next) = A dx + B dtau with the device's own step_derivatives
    within the parity bound; g' . step_jvp(d) = step_vjp(g') . d and the same for the integrator, within the sum of both calls' bounds."""
    torch = torch_cuda
    sys_, desc, hm = model_of(case)
    dt, nv, n = 0.02, desc.nv, desc.n_joints
    qh, qdh, qddh, tauh = state(sys_, B70)
    dsh = directions(B70, nv, 10)
    gah, gbh = cotangents(B70, nv, 11)
    q, qd, qdd0, tau, ga, gb = (dev(torch, x) for x in (qh, qdh, qddh, tauh, gah, gbh))
    ds = tuple(dev(torch, d) for d in dsh)
    f = dev(torch, random_wrenches(np.random.default_rng(33), B70, n))
    conds = conds_of(desc, qh)
    dot = lambda a, b: (a * b).sum(1, keepdim=True).cpu().numpy()
    qdd, dqdd, dqn, dqdn = hm.step_jvp(dt, q, qd, tau, *ds, GRAVITY, f)
    qdd_a, dqdd_a = hm.aba_jvp(q, qd, tau, *ds, GRAVITY, f)
    dqn_i, dqdn_i = hm.integrate_jvp(dt, qd, qdd_a, ds[0], ds[1], dqdd_a)
    assert all(torch.equal(a, b) for a, b in zip((qdd, dqdd, dqn, dqdn), (qdd_a, dqdd_a, dqn_i, dqdn_i)))
    _, _, _, A, Bm = hm.step_derivatives(dt, q, qd, tau, GRAVITY, f)
    x = torch.einsum("bij,bj->bi", A, torch.cat([ds[0], ds[1]], dim=1)) + torch.einsum("bij,bj->bi", Bm, ds[2])
    Ainf, Binf = (M.abs().amax(dim=(1, 2)).cpu().numpy() for M in (A, Bm))
    bound = step_bound(dsh, conds, n, U64, Ainf, Binf)
    held_rows(dqn.cpu().numpy(), x[:, :nv].cpu().numpy(), bound, "dq_next against the device matrices")
    held_rows(dqdn.cpu().numpy(), x[:, nv:].cpu().numpy(), bound, "dqd_next against the device matrices")
    # duality of the step: the VJP's own bound is |g'|_1 factor cond u max(1, |A|) per entry, contracted with the directions
    _, gq, gqd, gtau = hm.step_vjp(dt, q, qd, tau, ga, gb, GRAVITY, f)
    # (|g' . err| <= |g'|_1 bound on this side; on the other |err(gq, gqd) . dx| + |err(gtau) . dtau| sums to |g'|_1 bound as well)
    g1 = np.abs(gah).sum(axis=1) + np.abs(gbh).sum(axis=1)
    held_rows(dot(ga, dqn) + dot(gb, dqdn), dot(gq, ds[0]) + dot(gqd, ds[1]) + dot(gtau, ds[2]), 2.0 * g1 * bound, "g' . step_jvp against step_vjp . d")
    # duality of the integrator alone: 24 u abs-sums on both sides
    dqn, dqdn = hm.integrate_jvp(dt, qd, qdd0, *ds)
    gq, gqd, gqdd = hm.integrate_vjp(dt, qd, qdd0, ga, gb)
    _, _, sums_j = jc.integrate_jvp(desc, dt, qdh, qddh, *dsh)
    import step_vjp_check as svc
    _, _, _, sums_v = svc.integrate_vjp(desc, dt, qdh, qddh, gah, gbh)
    slack = 24.0 * U64 * ((np.abs(gah) * sums_j[0]).sum(axis=1) + (np.abs(gbh) * sums_j[1]).sum(axis=1)
                          + sum((np.abs(d) * s).sum(axis=1) for d, s in zip(dsh, sums_v)))
    lhs, rhs = dot(ga, dqn) + dot(gb, dqdn), dot(gq, ds[0]) + dot(gqd, ds[1]) + dot(gqdd, ds[2])
    # (the dot products themselves round too: nv terms each, relative to the sum of their absolute terms)
    size = (np.abs(gah * host(dqn, AOS)).sum(axis=1) + np.abs(gbh * host(dqdn, AOS)).sum(axis=1)
            + sum(np.abs(d * host(g, AOS)).sum(axis=1) for d, g in zip(dsh, (gq, gqd, gqdd))))
    held_rows(lhs, rhs, slack + 2.0 * nv * U64 * size, "g' . integrate_jvp against integrate_vjp . d")


# ------------------------------------------------------------------------------------------------ 4. exact cases
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_zero_step_zero_directions_and_null_directions(torch_cuda, dtype_name, layout):
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc, hm = model_of("humanoid30")
    q, qd, qdd, tau = (lay(dev(torch, x, dtype), layout) for x in state(sys_, B70))
    ds = tuple(lay(dev(torch, d, dtype), layout) for d in directions(B70, desc.nv, 11))
    f = lay(dev(torch, random_wrenches(np.random.default_rng(34), B70, desc.n_joints), dtype), layout)
    z = torch.zeros_like(qd)
    dqn, dqdn = hm.integrate_jvp(0.0, qd, qdd, *ds, layout)                                     # dt = 0: the identity
    assert bool((dqn == ds[0]).all()) and bool((dqdn == ds[1]).all())
    _, _, dqn, dqdn = hm.step_jvp(0.0, q, qd, tau, *ds, GRAVITY, f, layout)
    assert bool((dqn == ds[0]).all()) and bool((dqdn == ds[1]).all())
    assert not any(t.any() for t in hm.integrate_jvp(0.01, qd, qdd, z, z, z, layout))           # zero directions
    assert not any(t.any() for t in hm.step_jvp(0.01, q, qd, tau, z, z, z, GRAVITY, f, layout)[1:])
    for k in range(3):  # each direction alone, the others NULL: the bits of the call with zero tensors in their place
        alone = tuple(d if j == k else None for j, d in enumerate(ds))
        zeros = tuple(d if j == k else z for j, d in enumerate(ds))
        assert all(torch.equal(a, b) for a, b in zip(hm.integrate_jvp(0.01, qd, qdd, *alone, layout), hm.integrate_jvp(0.01, qd, qdd, *zeros, layout))), k
        got, ref = hm.step_jvp(0.01, q, qd, tau, *alone, GRAVITY, f, layout), hm.step_jvp(0.01, q, qd, tau, *zeros, GRAVITY, f, layout)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), k


# ------------------------------------------------------------------------------------------------ 5. cover, NULL outputs
@functools.lru_cache(maxsize=None)
def _cover_reference(case, B, dt):
    """The rows that cover every group of a batch of B, their directions and wrenches, and the checker's outputs on them: once per
    (model, batch), shared by the layouts and the output selections, never modified."""
    sys_, desc, _ = model_of(case)
    rows = DistinctRows(sys_, 256, seed=29)
    idx = group_cover(B, None)
    ds_host = directions(64, desc.nv, 13)
    f_host = random_wrenches(np.random.default_rng(24), 64, desc.n_joints)
    qi, qdi, _, taui = rows.rows(idx)
    di = tuple(d[idx % 64] for d in ds_host)
    return rows, idx, ds_host, f_host, di, conds_of(desc, qi), jc.step_jvp(desc, dt, qi, qdi, taui, *di, GRAVITY, f_host[idx % 64])


def _cover_step(torch, case, B, layout, keep, dt=0.02):
    """B distinct rows, poisoned outputs with a guard row behind them, every row group against the checker; keep: the outputs asked for
    among (qdd, dqdd, dq_next, dqd_next)."""
    sys_, desc, hm = model_of(case)
    rows, idx, ds_host, f_host, di, conds, ref = _cover_reference(case, B, dt)
    q, qd, _, tau = rows.device(torch, B)
    nv = desc.nv
    period = torch.arange(B, device="cuda") % 64
    ds = tuple(dev(torch, d)[period].contiguous() for d in ds_host)
    f = dev(torch, f_host)[period].contiguous()
    outs, guards = [], []
    for k in range(4):
        if k not in keep:
            outs.append(None), guards.append(None)
            continue
        o, g = poisoned(torch, B, (nv,), torch.float64) if layout == AOS else poisoned(torch, nv, (B,), torch.float64)
        outs.append(o), guards.append(g)
    hm.step_jvp(dt, *(lay(x, layout) for x in (q, qd, tau) + ds), GRAVITY, lay(f, layout), layout, out=tuple(outs))
    torch.cuda.synchronize()
    qdd_ref, dqdd, dqn, dqdn, _, (Ainf, Binf), scales = ref
    sb = step_bound(di, conds, desc.n_joints, U64, Ainf, Binf)
    bounds = [None, aba_bound(di, scales, conds, desc.n_joints, U64), sb, sb]
    take = torch.as_tensor(idx, device="cuda")
    for k, (o, g, r, b) in enumerate(zip(outs, guards, (qdd_ref, dqdd, dqn, dqdn), bounds)):
        if o is None:
            continue
        assert torch.isnan(g).all(), f"output {k}: wrote past the last row"
        assert not torch.isnan(o).any(), f"output {k}: rows left unwritten (NaN)"
        got = (o if layout == AOS else o.t())[take].cpu().numpy()
        if b is None:
            close_aba(got, r, None, desc.n_joints, U64, label="qdd", conds=conds)
        else:
            held_rows(got, r, b, f"output {k}")


@pytest.mark.parametrize("case", ["humanoid30", "onedof_tree"])
@pytest.mark.parametrize("keep", [(0, 1, 2, 3), (1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2), (1,), (3,)])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_each_optional_output_null_in_turn(torch_cuda, case, keep, layout):
    _cover_step(torch_cuda, case, 64 * 5 + 3, layout, keep)


@pytest.mark.parametrize("case,B", [("humanoid30", 8192 + 37), ("onedof_tree", 4096), ("humanoid30", 64 * 3 + 1)])
def test_step_covers_every_row_group(torch_cuda, case, B):
    _cover_step(torch_cuda, case, B, AOS if B % 2 else SOA, (0, 1, 2, 3))


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_integrate_jvp_device_filling_batch_and_null_outputs(torch_cuda, layout):
    """arm7, 2 * 8 * CUs * 64 + 64 + 37 rows: every row group of the elementwise kernel, each output NULL in turn."""
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    sys_, desc, hm = model_of("arm7")
    B, nv, dt = 2 * 8 * cus * 64 + 64 + 37, desc.nv, 0.05
    rows = DistinctRows(sys_, 256, seed=29)
    _, qd, qdd, _ = rows.device(torch, B)
    idx = group_cover(B, 8 * cus)
    ds_host = directions(64, nv, 13)
    period = torch.arange(B, device="cuda") % 64
    ds = tuple(dev(torch, d)[period].contiguous() for d in ds_host)
    _, qdi, qddi, _ = rows.rows(idx)
    *ref, sums = jc.integrate_jvp(desc, dt, qdi, qddi, *(d[idx % 64] for d in ds_host))
    take = torch.as_tensor(idx, device="cuda")
    for keep in ((0, 1), (0,), (1,)):
        pairs = [poisoned(torch, B, (nv,), torch.float64) if layout == AOS else poisoned(torch, nv, (B,), torch.float64) for _ in range(2)]
        outs = tuple(p[0] if k in keep else None for k, p in enumerate(pairs))
        hm.integrate_jvp(dt, *(lay(x, layout) for x in (qd, qdd) + ds), layout, out=outs)
        torch.cuda.synchronize()
        for k in keep:
            o, g = pairs[k]
            assert torch.isnan(g).all() and not torch.isnan(o).any(), k
            held_entries((o if layout == AOS else o.t())[take].cpu().numpy(), ref[k], sums[k], U64, f"cover integrate_jvp output {k}")


# ------------------------------------------------------------------------------------------------ 6. scattered index maps
@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if dtype_name == "float32" else np.float64
    dt = float(np.float32(0.02))
    q, qd, qdd, tau = DistinctRows(sys_, 16, seed=51).rows(np.arange(70), np_dt)
    ds = tuple(d.astype(np_dt).astype(np.float64) for d in directions(70, d0.nv, 52))
    f = random_wrenches(np.random.default_rng(53), 70, d0.n_joints).astype(np_dt).astype(np.float64)
    conds = conds_of(d0, q)
    assert conds.max() < 1.0e8
    return dt, (q, qd, qdd, tau, ds, f), jc.integrate_jvp(d0, dt, qd, qdd, *ds), jc.step_jvp(d0, dt, q, qd, tau, *ds, GRAVITY, f), conds


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """integrate_jvp and step_jvp on a description with scattered maps (with holes: unowned indices holding 7.0 in every input, the
    directions included) against the checker on the IDENTITY description: directions go in and tangents come back through the DoF map;
    unowned outputs are exact zeros, the guards stay poisoned, the unmoved read misses the reference."""
    torch = torch_cuda
    dtype, unit = getattr(torch, dtype_name), (U32 if dtype_name == "float32" else U64)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, n = hp.scattered_model(d, model), 70, d.nv, d0.n_joints
    dt, (q, qd, qdd, tau, ds, f), (rn, rdn, sums), step_ref, conds = _scattered_reference(model, dtype_name)
    is_soa = layout == SOA
    put = lambda x: lay(dev(torch, x, dtype), layout)
    tq = put(hp.to_q(q, pq, d.nq))
    tqd, tqdd, ttau, t1, t2, t3 = (put(hp.to_v(x, pv, nv)) for x in (qd, qdd, tau) + ds)
    tf = put(f.reshape(B, -1))
    outs, guards = hp.poisoned_set(torch, B, [(nv,)] * 6, dtype, is_soa)
    hm.integrate_jvp(dt, tqd, tqdd, t1, t2, t3, layout, out=(outs[0], outs[1]))
    hm.step_jvp(dt, tq, tqd, ttau, t1, t2, t3, GRAVITY, tf, layout, out=tuple(outs[2:]))
    torch.cuda.synchronize()
    hp.guards_intact(guards, "step jvp")
    got = [hp.rows_of(o, B, (nv,), is_soa) for o in outs]
    for g, r, s, name in zip(got[:2], (rn, rdn), sums, ("dq_next", "dqd_next")):
        back, free = hp.from_v(g, pv)
        assert not free.any(), name
        held_entries(back, r, s, unit, f"scattered integrate_jvp {name}")
        hp.assert_misses(hp.keep_order(g, pv), r, name)
    qdd_ref, dqdd, dqn, dqdn, _, (Ainf, Binf), scales = step_ref
    sb = step_bound(ds, conds, n, unit, Ainf, Binf)
    close_aba(hp.from_v(got[2], pv)[0], qdd_ref, None, n, unit, label="scattered qdd", conds=conds)
    for g, r, b, name in zip(got[3:], (dqdd, dqn, dqdn), (aba_bound(ds, scales, conds, n, unit), sb, sb), ("dqdd", "dq_next", "dqd_next")):
        back, free = hp.from_v(g, pv)
        assert not free.any(), name
        held_rows(back, r, b, f"scattered step_jvp {name}")
        hp.assert_misses(hp.keep_order(g, pv), r, "step " + name)


# ------------------------------------------------------------------------------------------------ 7. plumbing
def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() and a first call all four forward-mode
    calls are captured into one graph (they allocate nothing) and the replay gives the bits of the direct calls, also on changed inputs."""
    torch = torch_cuda
    sys_, desc, hm = model_of("humanoid30")
    B, dt = 1000, 0.01
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    ds = tuple(dev(torch, d) for d in directions(B, desc.nv))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))

    def direct():
        r = (hm.rnea_jvp(q, qd, qdd, *ds, GRAVITY, f),) + hm.aba_jvp(q, qd, tau, *ds, GRAVITY, f)[1:] + hm.integrate_jvp(dt, qd, qdd, *ds) \
            + hm.step_jvp(dt, q, qd, tau, *ds, GRAVITY, f)[2:]
        torch.cuda.synchronize()
        return r

    ref = direct()
    view = hm.context()
    view.reserve(B)
    outs = tuple(torch.empty_like(t) for t in ref)

    def calls():
        view.rnea_jvp(q, qd, qdd, *ds, GRAVITY, f, out=outs[0])
        view.aba_jvp(q, qd, tau, *ds, GRAVITY, f, out=(None, outs[1]))  # qdd and the right-hand side in the context's scratch
        view.integrate_jvp(dt, qd, qdd, *ds, out=(outs[2], outs[3]))
        view.step_jvp(dt, q, qd, tau, *ds, GRAVITY, f, out=(None, None, outs[4], outs[5]))  # three vectors of scratch

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        calls()
        view.check(s.cuda_stream)
        assert all(torch.equal(a, b) for a, b in zip(outs, ref))
        for t in outs:
            t.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            calls()
    torch.cuda.synchronize()
    assert not any(t.any() for t in outs)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))
    q.copy_(dev(torch, state(sys_, B, seed=6)[0])), ds[0].copy_(dev(torch, directions(B, desc.nv, 14)[0]))
    ref2 = direct()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, ref2)) and not torch.equal(ref2[0], ref[0])
    view.close()


def test_wrong_shapes_overlaps_and_source_joints_are_refused(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = HipModel(desc), 10, desc.nv, desc.n_joints
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    ds = tuple(dev(torch, d) for d in directions(B, nv))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(n * 6, B)):
        with pytest.raises(_lib.MecanoHipError):
            hm.step_jvp(0.01, q, qd, tau, *ds, GRAVITY, bad_f)
    for k in range(3):
        bad = tuple(z(B, nv + 1) if j == k else d for j, d in enumerate(ds))
        with pytest.raises(_lib.MecanoHipError):
            hm.integrate_jvp(0.01, qd, qdd, *bad)
        with pytest.raises(_lib.MecanoHipError):
            hm.step_jvp(0.01, q, qd, tau, *bad, GRAVITY)
    for method, args in ((hm.integrate_jvp, (0.01, qd, qdd)), (hm.step_jvp, (0.01, q, qd, tau))):
        with pytest.raises(_lib.MecanoHipError):
            method(*args, None, None, None)
        with pytest.raises(_lib.MecanoHipError):
            method(float("inf"), *args[1:], *ds)
    with pytest.raises(_lib.MecanoHipError):
        hm.integrate_jvp(0.01, qd, qdd, *ds, out=(None, None))
    with pytest.raises(_lib.MecanoHipError):
        hm.step_jvp(0.01, q, qd, tau, *ds, GRAVITY, None, out=(z(B, nv), None, None, None))
    vec = (B, nv)
    check_bad_outputs(torch, [vec, vec], lambda out: hm.integrate_jvp(0.01, qd, qdd, *ds, out=out))
    check_bad_outputs(torch, [vec, vec, vec, vec], lambda out: hm.step_jvp(0.01, q, qd, tau, *ds, GRAVITY, None, out=out))
    # every forbidden overlap: an output on an input (q has nq = nv here), directions included, two outputs on each other
    nan = lambda: torch.full((B, nv), float("nan"), dtype=torch.float64, device="cuda")
    for method, head, inputs, tail, n_out in ((hm.integrate_jvp, (0.01,), (qd, qdd) + ds, (), 2), (hm.step_jvp, (0.01,), (q, qd, tau) + ds, (GRAVITY, None), 4)):
        before = [t.clone() for t in inputs]
        for k in range(n_out):
            for t in inputs:
                outs = [nan() for _ in range(n_out)]
                outs[k] = t
                with pytest.raises(_lib.MecanoHipError):
                    method(*head, *inputs, *tail, out=tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for j, o in enumerate(outs) if j != k)
            for j in range(k):
                outs = [nan() for _ in range(n_out)]
                outs[k] = outs[j]
                with pytest.raises(_lib.MecanoHipError):
                    method(*head, *inputs, *tail, out=tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for o in outs)
        assert all(torch.equal(a, b) for a, b in zip(inputs, before))
    modes = [0] * n
    modes[2] = 1
    hm.set_joint_source_modes(modes)
    outs = tuple(nan() for _ in range(4))
    with pytest.raises(_lib.MecanoHipError):
        hm.step_jvp(0.01, q, qd, tau, *ds, GRAVITY, None, out=outs)
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    hm.integrate_jvp(0.01, qd, qdd, *ds)  # joint source modes play no part in the integrator's tangent map
    hm.set_joint_source_modes(None)
