"""mh_rnea_jvp_* / mh_aba_jvp_* on the device against the CPU checker (tests/dynamics_jvp_check.py: the matrices of
tests/dynamics_derivatives_check.py times the directions, pinned by tests/test_dynamics_jvp_cpu.py) and against the device's own
neighbours (rnea_derivatives, aba_derivatives, rnea_vjp, aba_vjp, gravity_gradient).

Bounds.  An output entry is a sum of contractions sum_j D_ij d_j, so the project's per-entry bound of a matrix, TOL max(1, |D_ref|_inf)
(helpers.close), sums to |d|_1 TOL max(1, |D_ref|_inf) per configuration and direction, and over the three directions -- as rnea_bounds /
aba_bounds of test_gpu_dynamics_vjp.py sum over a cotangent.  The forward form takes the per-row factor of helpers.close_aba in place of
TOL: 8 sqrt(8 * 3 n) cond_inf(H) u, cond from the oracle's H.  fp32: helpers.f32_forward_tol(3 n) in place of TOL, u = 2^-24, the checker
fed the fp32-rounded inputs.  Every check records achieved / bound (helpers.record_parity)."""
import functools

import numpy as np
import pytest

import dynamics_jvp_check as jc
import helpers as hp
from helpers import DistinctRows, check_bad_outputs, close_aba, f32_aba_forward_factor, f32_forward_tol, group_cover, poisoned
from mecano_amd import random_tools as rt
from test_gpu_dynamics_vjp import AOS, SOA, TOL, TREE_ROWS, U32, U64, conds_of, cotangent, dev, held, host, soa, state
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def directions(B, nv, seed=8):
    return tuple(cotangent(B, nv, seed + k) for k in range(3))


def l1(d, B):
    return np.zeros(B) if d is None else np.abs(d).sum(axis=1)


def rnea_bound(ds, scales, tol=TOL):
    B = len(scales[0])
    return sum(l1(d, B) * np.maximum(1.0, s) for d, s in zip(ds, scales)) * tol


def aba_bound(ds, scales, conds, n_joints, unit):
    B = len(scales[0])
    return sum(l1(d, B) * np.maximum(1.0, s) for d, s in zip(ds, scales)) * f32_aba_forward_factor(3 * n_joints) * conds * unit


def call(torch, method, arrays, f, layout, dtype=None, gravity=GRAVITY, **kw):
    """hm.rnea_jvp / hm.aba_jvp on host arrays (q, qd, qdd | tau, d1, d2, d3; any direction None): the outputs as AoS-shaped fp64 arrays."""
    args = [dev(torch, x, dtype) for x in arrays] + [dev(torch, f, dtype)]
    if layout == SOA:
        args = [soa(x) for x in args]
    out = method(*args[:6], gravity, args[6], layout, **kw)
    torch.cuda.synchronize()
    return host(out, layout) if not isinstance(out, tuple) else tuple(host(t, layout) for t in out)


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
    q, qd, qdd, tau = state(sys_, B)
    ds = directions(B, desc.nv)
    f = None if wrenches == "none" else random_wrenches(np.random.default_rng(21), B, desc.n_joints)
    got = call(torch_cuda, hm.rnea_jvp, (q, qd, qdd) + ds, f, layout)
    ref, scales = jc.rnea_jvp(desc, q, qd, qdd, *ds, GRAVITY, f)
    held(got, ref, rnea_bound(ds, scales), "dtau")
    qdd_d, got = call(torch_cuda, hm.aba_jvp, (q, qd, tau) + ds, f, layout)
    qdd_ref, ref, scales = jc.aba_jvp(desc, q, qd, tau, *ds, GRAVITY, f)
    conds = conds_of(desc, q)
    close_aba(qdd_d, qdd_ref, None, desc.n_joints, U64, label="qdd", conds=conds)
    held(got, ref, aba_bound(ds, scales, conds, desc.n_joints, U64), "dqdd")


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_fp32_matches_checker(torch_cuda, case):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q, qd, qdd, tau = (x.astype(np.float32) for x in state(sys_, B))
    ds = tuple(d.astype(np.float32) for d in directions(B, desc.nv))
    f = random_wrenches(np.random.default_rng(22), B, desc.n_joints).astype(np.float32)
    q64, qd64, qdd64, tau64, f64 = (x.astype(np.float64) for x in (q, qd, qdd, tau, f))
    ds64 = tuple(d.astype(np.float64) for d in ds)
    ref, scales = jc.rnea_jvp(desc, q64, qd64, qdd64, *ds64, GRAVITY, f64)
    qdd_ref, ref_f, scales_f = jc.aba_jvp(desc, q64, qd64, tau64, *ds64, GRAVITY, f64)
    conds = conds_of(desc, q64)
    for layout in (AOS, SOA):
        got = call(torch, hm.rnea_jvp, (q, qd, qdd) + ds, f, layout, dtype=torch.float32)
        held(got, ref, rnea_bound(ds64, scales, f32_forward_tol(3 * desc.n_joints)), f"fp32 dtau layout {layout}")
        qdd_d, got = call(torch, hm.aba_jvp, (q, qd, tau) + ds, f, layout, dtype=torch.float32)
        close_aba(qdd_d, qdd_ref, None, desc.n_joints, U32, label=f"fp32 qdd layout {layout}", conds=conds)
        held(got, ref_f, aba_bound(ds64, scales_f, conds, desc.n_joints, U32), f"fp32 dqdd layout {layout}")


def test_tree128_rows(torch_cuda):
    """The committed 128-body benchmark tree, nv = 323, fp64 AoS: both calls on the rows TREE_ROWS; every row free of NaN."""
    from mecano_amd.engine import HipModel
    sys_ = rt.committedBenchmarkSystems()["tree128"]
    desc = sys_.toModelDesc()
    assert desc.nv == 323
    hm, B = HipModel(desc), 70
    q, qd, qdd, tau = state(sys_, B)
    ds = directions(B, desc.nv)
    f = random_wrenches(np.random.default_rng(22), B, desc.n_joints)
    got = call(torch_cuda, hm.rnea_jvp, (q, qd, qdd) + ds, f, AOS)
    ref, scales = jc.rnea_jvp(desc, q, qd, qdd, *ds, GRAVITY, f, rows=TREE_ROWS)
    held(got, ref, rnea_bound(ds, scales), "tree128 dtau", rows=TREE_ROWS)
    qdd_d, got = call(torch_cuda, hm.aba_jvp, (q, qd, tau) + ds, f, AOS)
    qdd_ref, ref, scales = jc.aba_jvp(desc, q, qd, tau, *ds, GRAVITY, f, rows=TREE_ROWS)
    conds = np.ones(B)
    conds[TREE_ROWS] = conds_of(desc, q[TREE_ROWS])
    assert not np.isnan(qdd_d).any()
    close_aba(qdd_d[TREE_ROWS], qdd_ref[TREE_ROWS], None, desc.n_joints, U64, label="tree128 qdd", conds=conds[TREE_ROWS])
    held(got, ref, aba_bound(ds, scales, conds, desc.n_joints, U64), "tree128 dqdd", rows=TREE_ROWS)


# ------------------------------------------------------------------------------------------------ device against device
@pytest.mark.parametrize("case", ["humanoid30", "planar", "spherical"])
def test_contracts_the_device_matrices_and_is_dual_to_the_vjp(torch_cuda, case):
    """dtau = D dq + D' dqd + H dqdd with the matrices of rnea_derivatives and crba on the same inputs, dqdd likewise with aba_derivatives,
    within the parity bound; u . jvp(d) = vjp(u) . d within the sum of both calls' bounds."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B, nv, n = HipModel(desc), 70, desc.nv, desc.n_joints
    qh, qdh, qddh, tauh = state(sys_, B)
    dsh, uh = directions(B, nv), cotangent(B, nv, 12)
    q, qd, qdd, tau, u = (dev(torch, x) for x in (qh, qdh, qddh, tauh, uh))
    ds = tuple(dev(torch, d) for d in dsh)
    f = dev(torch, random_wrenches(np.random.default_rng(23), B, n))
    conds = conds_of(desc, qh)
    amax = lambda Ms: [M.abs().amax(dim=(1, 2)).cpu().numpy() for M in Ms]
    dot = lambda a, b: (a * b).sum(1, keepdim=True).cpu().numpy()
    u1 = np.abs(uh).sum(axis=1)

    dtau = hm.rnea_jvp(q, qd, qdd, *ds, GRAVITY, f)
    _, Dq, Dv = hm.rnea_derivatives(q, qd, qdd, GRAVITY, f)
    Ms = (Dq, Dv, hm.crba(q))
    bound = rnea_bound(dsh, amax(Ms))
    ref = sum(torch.einsum("bij,bj->bi", M, d) for M, d in zip(Ms, ds))
    held(dtau.cpu().numpy(), ref.cpu().numpy(), bound, "dtau against the device matrices")
    # |u . err(dtau)| <= |u|_1 bound; |err(g_k) . d_k| <= |d_k|_1 |u|_1 TOL max(1, |D_k|), which sums to |u|_1 bound as well
    gs = hm.rnea_vjp(q, qd, qdd, u, GRAVITY, f)
    held(dot(u, dtau), sum(dot(g, d) for g, d in zip(gs, ds)), 2.0 * u1 * bound, "u . rnea_jvp against rnea_vjp . d")

    qdd_j, dqdd = hm.aba_jvp(q, qd, tau, *ds, GRAVITY, f)
    qdd_m, Eq, Ev, Hinv = hm.aba_derivatives(q, qd, tau, GRAVITY, f)
    Ms = (Eq, Ev, Hinv)
    bound = aba_bound(dsh, amax(Ms), conds, n, U64)
    ref = sum(torch.einsum("bij,bj->bi", M, d) for M, d in zip(Ms, ds))
    held(dqdd.cpu().numpy(), ref.cpu().numpy(), bound, "dqdd against the device matrices")
    assert torch.equal(qdd_j, hm.aba(q, qd, tau, GRAVITY, f))
    gs = hm.aba_vjp(q, qd, tau, u, GRAVITY, f)[1:]
    held(dot(u, dqdd), sum(dot(g, d) for g, d in zip(gs, ds)), 2.0 * u1 * bound, "u . aba_jvp against aba_vjp . d")


# ------------------------------------------------------------------------------------------------ exact cases
def test_exact_cases(torch_cuda):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 100
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    dsh = directions(B, desc.nv)
    ds, z = tuple(dev(torch, d) for d in dsh), torch.zeros_like(qd)
    f = dev(torch, random_wrenches(np.random.default_rng(25), B, desc.n_joints, always=True))
    for layout in (AOS, SOA):
        lay = (lambda x: x) if layout == AOS else soa
        a_q, a_qd, a_qdd, a_tau, a_z, a_f = (lay(x) for x in (q, qd, qdd, tau, z, f))
        a_ds = tuple(lay(d) for d in ds)
        assert not hm.rnea_jvp(a_q, a_qd, a_qdd, a_z, a_z, a_z, GRAVITY, a_f, layout).any()              # zero directions
        assert not hm.aba_jvp(a_q, a_qd, a_tau, a_z, a_z, a_z, GRAVITY, a_f, layout)[1].any()
        for k in range(3):  # each direction alone, the others NULL: the bits of the call with zero tensors in their place
            alone = tuple(d if j == k else None for j, d in enumerate(a_ds))
            zeros = tuple(d if j == k else a_z for j, d in enumerate(a_ds))
            assert torch.equal(hm.rnea_jvp(a_q, a_qd, a_qdd, *alone, GRAVITY, a_f, layout), hm.rnea_jvp(a_q, a_qd, a_qdd, *zeros, GRAVITY, a_f, layout)), k
            got, ref = hm.aba_jvp(a_q, a_qd, a_tau, *alone, GRAVITY, a_f, layout), hm.aba_jvp(a_q, a_qd, a_tau, *zeros, GRAVITY, a_f, layout)
            # (dtau alone runs no sweep; with zero dq and dqd the sweep hands dtau - 0 on)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), k
        off = hm.rnea_jvp(a_q, None, a_qdd, a_ds[0], None, a_ds[2], GRAVITY, a_f, layout, consider_coriolis=False)
        assert torch.equal(off, hm.rnea_jvp(a_q, a_z, a_qdd, a_ds[0], a_z, a_ds[2], GRAVITY, a_f, layout)) and off.any()
        assert torch.equal(off, hm.rnea_jvp(a_q, None, a_qdd, a_ds[0], a_ds[1], a_ds[2], GRAVITY, a_f, layout, consider_coriolis=False))
        off = hm.rnea_jvp(a_q, a_qd, None, *a_ds, GRAVITY, a_f, layout, consider_accelerations=False)
        assert torch.equal(off, hm.rnea_jvp(a_q, a_qd, a_z, *a_ds, GRAVITY, a_f, layout))
        # only dtau, with qdd asked for: the bits of aba_vjp's gtau for w = dtau
        qdd_j, dqdd = hm.aba_jvp(a_q, a_qd, a_tau, None, None, a_ds[2], GRAVITY, a_f, layout)
        qdd_v, _, _, gtau = hm.aba_vjp(a_q, a_qd, a_tau, a_ds[2], GRAVITY, a_f, layout)
        assert torch.equal(dqdd, gtau) and torch.equal(qdd_j, qdd_v)
        only = hm.aba_jvp(a_q, a_qd, a_tau, None, None, a_ds[2], GRAVITY, a_f, layout, out=(None, torch.empty_like(a_qd)))[1]
        assert torch.equal(only, gtau)
    for fe in (None, f):  # at rest: (gravity gradient) dq
        got = hm.rnea_jvp(q, z, z, ds[0], None, None, GRAVITY, fe).cpu().numpy()
        grad = hm.gravity_gradient(q, GRAVITY, fe)[1]
        ref = torch.einsum("bij,bj->bi", grad, ds[0]).cpu().numpy()
        held(got, ref, rnea_bound((dsh[0],), [grad.abs().amax(dim=(1, 2)).cpu().numpy()]), "at rest vs gravity_gradient")


def test_forward_form_hands_the_callers_switches_to_forward_dynamics_only(torch_cuda):
    """mh_aba_jvp_* handed consider_coriolis = 0 through the C ABI (the engine never does): qdd_out has the bits of mh_aba_* with the same
    options, and dqdd those of H^-1 (dtau - rnea_jvp(q, qd, qdd_out, dq, dqd, 0)) with both switches on, as mh_aba_vjp_* composes it."""
    import ctypes

    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 197
    q, qd, _, tau = (dev(torch, x) for x in state(sys_, B))
    ds = tuple(dev(torch, d) for d in directions(B, desc.nv))
    f = dev(torch, random_wrenches(np.random.default_rng(31), B, desc.n_joints))
    qdd, dqdd, qdd_aba = (torch.full_like(qd, float("nan")) for _ in range(3))
    g, ra = hm._root(GRAVITY)
    opts = hm._options(AOS, False, True, torch.cuda.current_stream().cuda_stream, root_acceleration=ra)
    lib = _lib.load()
    _lib.check(lib.mh_aba_jvp_f64(hm._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, f.data_ptr(), *(d.data_ptr() for d in ds),
                                  ctypes.byref(opts), qdd.data_ptr(), dqdd.data_ptr()))
    _lib.check(lib.mh_aba_f64(hm._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, f.data_ptr(), ctypes.byref(opts), qdd_aba.data_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(qdd).all() and torch.equal(qdd, qdd_aba)
    r = ds[2] - hm.rnea_jvp(q, qd, qdd, ds[0], ds[1], None, GRAVITY, f)
    assert torch.equal(dqdd, hm.aba_vjp(q, qd, tau, r, GRAVITY, f, out=(None, None, None, torch.empty_like(qd)))[3])


# ------------------------------------------------------------------------------------------------ scattered index maps
@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    """States and directions in the identity description's index space and the checker's outputs on them: once per model and precision,
    shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if dtype_name == "float32" else np.float64
    q, qd, qdd, tau = DistinctRows(sys_, 16, seed=51).rows(np.arange(70), np_dt)
    ds = tuple(d.astype(np_dt).astype(np.float64) for d in directions(70, d0.nv, 52))
    f = random_wrenches(np.random.default_rng(53), 70, d0.n_joints).astype(np_dt).astype(np.float64)
    conds = conds_of(d0, q)
    assert conds.max() < 1.0e8
    return (q, qd, qdd, tau, ds, f), jc.rnea_jvp(d0, q, qd, qdd, *ds, GRAVITY, f), jc.aba_jvp(d0, q, qd, tau, *ds, GRAVITY, f), conds


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """rnea_jvp and aba_jvp on a description whose maps send every DoF and every configuration entry somewhere else (with holes: two
    indices of each space owned by no joint, holding 7.0 in every input, the directions included), against the checker on the IDENTITY
    description: directions go in and tangents come back through the DoF map and meet this file's bounds; the tangents at unowned indices
    are exact zeros, the guard rows stay poisoned; read without moving them back the outputs miss the reference by more than 1e-3."""
    torch = torch_cuda
    dtype, unit = getattr(torch, dtype_name), (U32 if dtype_name == "float32" else U64)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, n = hp.scattered_model(d, model), 70, d.nv, d0.n_joints
    (q, qd, qdd, tau, ds, f), (ref_i, scales_i), (qdd_ref, ref_f, scales_f), conds = _scattered_reference(model, dtype_name)
    is_soa = layout == SOA
    lay = soa if is_soa else (lambda x: x)
    tq = lay(dev(torch, hp.to_q(q, pq, d.nq), dtype))
    tqd, tqdd, ttau, t1, t2, t3 = (lay(dev(torch, hp.to_v(x, pv, nv), dtype)) for x in (qd, qdd, tau) + ds)
    tf = lay(dev(torch, f, dtype))
    if holes:
        free = np.setdiff1d(np.arange(nv), pv)
        assert len(free) and np.all(hp.to_v(ds[0], pv, nv)[:, free] == 7.0)
    outs, guards = hp.poisoned_set(torch, B, [(nv,)] * 3, dtype, is_soa)
    hm.rnea_jvp(tq, tqd, tqdd, t1, t2, t3, GRAVITY, tf, layout, out=outs[0])
    hm.aba_jvp(tq, tqd, ttau, t1, t2, t3, GRAVITY, tf, layout, out=(outs[1], outs[2]))
    torch.cuda.synchronize()
    hp.guards_intact(guards, "jvp")
    dtau, qdd_d, dqdd = (hp.rows_of(o, B, (nv,), is_soa) for o in outs)
    bound_i = rnea_bound(ds, scales_i, TOL if dtype_name == "float64" else f32_forward_tol(3 * n))
    bound_f = aba_bound(ds, scales_f, conds, n, unit)
    for g, r, b, name in ((dtau, ref_i, bound_i, "dtau"), (dqdd, ref_f, bound_f, "dqdd")):
        back, free = hp.from_v(g, pv)
        assert not free.any(), name  # exact zeros, and written
        held(back, r, b, f"scattered {name}")
        hp.assert_misses(hp.keep_order(g, pv), r, name)
    close_aba(hp.from_v(qdd_d, pv)[0], qdd_ref, None, n, unit, label="scattered qdd", conds=conds)


# ------------------------------------------------------------------------------------------------ cover of batches
def _cover_case(torch, sys_, desc, B, grid, layout, with_f, forward=False, skip=None):
    """B distinct rows, poisoned outputs with a guard row behind them, every row group checked against the checker; forward: aba_jvp, with
    `skip` = 0 for qdd_out NULL."""
    from mecano_amd.engine import HipModel
    hm = HipModel(desc)
    rows = DistinctRows(sys_, 256, seed=29)
    q, qd, qdd, tau = rows.device(torch, B)
    idx = group_cover(B, grid)
    nv = desc.nv
    ds_host = directions(64, nv, 13)
    f_host = random_wrenches(np.random.default_rng(24), 64, desc.n_joints) if with_f else None
    period = torch.arange(B, device="cuda") % 64
    ds = tuple(dev(torch, d)[period].contiguous() for d in ds_host)
    f = dev(torch, f_host)[period].contiguous() if with_f else None
    outs, guards = [], []
    for k in range(2 if forward else 1):
        if forward and k == skip:
            outs.append(None), guards.append(None)
            continue
        o, g = poisoned(torch, B, (nv,), torch.float64) if layout == AOS else poisoned(torch, nv, (B,), torch.float64)
        outs.append(o), guards.append(g)
    x3 = tau if forward else qdd
    lay = (lambda x: x) if layout == AOS else soa
    args = (lay(q), lay(qd), lay(x3)) + tuple(lay(d) for d in ds) + (GRAVITY, lay(f))
    if forward:
        hm.aba_jvp(*args, layout, out=tuple(outs))
    else:
        hm.rnea_jvp(*args, layout, out=outs[0])
    torch.cuda.synchronize()
    qi, qdi, qddi, taui = rows.rows(idx)
    di, fi = tuple(d[idx % 64] for d in ds_host), None if f_host is None else f_host[idx % 64]
    if forward:
        conds = conds_of(desc, qi)
        qdd_ref, ref, scales = jc.aba_jvp(desc, qi, qdi, taui, *di, GRAVITY, fi)
        refs, bounds = [qdd_ref, ref], [None, aba_bound(di, scales, conds, desc.n_joints, U64)]
    else:
        ref, scales = jc.rnea_jvp(desc, qi, qdi, qddi, *di, GRAVITY, fi)
        refs, bounds = [ref], [rnea_bound(di, scales)]
    take = torch.as_tensor(idx, device="cuda")
    for k, (o, g, r, b) in enumerate(zip(outs, guards, refs, bounds)):
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


@pytest.mark.parametrize("case,B", [("humanoid30", 8192 + 37), ("onedof_tree", 4096), ("humanoid30", 64 * 3 + 1), ("onedof_tree", 64 * 3 + 1)])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_ragged_and_full_batches_cover_every_row_group(torch_cuda, case, B, layout):
    """(The parts split is taken at 64 * 3 + 1.)"""
    sys_, desc = make_case(case)
    _cover_case(torch_cuda, sys_, desc, B, None, layout, with_f=(B % 2 == 1))


@pytest.mark.parametrize("case", ["humanoid30", "onedof_tree"])
@pytest.mark.parametrize("skip", [None, 0])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_with_and_without_qdd_out(torch_cuda, case, skip, layout):
    """64 * 5 + 3 rows; qdd_out NULL: qdd and the right-hand side both in the context's scratch."""
    sys_, desc = make_case(case)
    _cover_case(torch_cuda, sys_, desc, 64 * 5 + 3, None, layout, with_f=True, forward=True, skip=skip)


# ------------------------------------------------------------------------------------------------ plumbing
def test_wrong_shapes_overlaps_and_source_joints_are_refused(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = HipModel(desc), 10, desc.nv, desc.n_joints
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    ds = tuple(dev(torch, d) for d in directions(B, nv))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(B, n, 5), z(n * 6, B)):
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_jvp(q, qd, qdd, *ds, GRAVITY, bad_f)
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_jvp(q, qd, tau, *ds, GRAVITY, bad_f)
    for k in range(3):  # a direction of a wrong shape, every direction None
        bad = tuple(z(B, nv + 1) if j == k else d for j, d in enumerate(ds))
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_jvp(q, qd, qdd, *bad, GRAVITY)
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_jvp(q, qd, tau, *bad, GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_jvp(q, qd, qdd, None, None, None, GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_jvp(q, qd, tau, None, None, None, GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_jvp(q, qd, None, *ds, GRAVITY)
    for bad_out in ((None, None), (z(B, nv), None), (z(B, nv + 1), z(B, nv)), (z(B, nv),)):
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_jvp(q, qd, tau, *ds, GRAVITY, None, out=bad_out)
    vec = (B, nv)
    check_bad_outputs(torch, vec, lambda out: hm.rnea_jvp(q, qd, qdd, *ds, GRAVITY, None, out=out))
    check_bad_outputs(torch, [vec, vec], lambda out: hm.aba_jvp(q, qd, tau, *ds, GRAVITY, None, out=out))
    # every forbidden overlap: an output on an input (q has nq = nv here), directions included, two outputs on each other
    nan = lambda: torch.full((B, nv), float("nan"), dtype=torch.float64, device="cuda")
    inputs = (q, qd, qdd) + ds
    before = [t.clone() for t in inputs]
    for t in inputs:
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_jvp(*inputs, GRAVITY, None, out=t)
    inputs = (q, qd, tau) + ds
    for k in range(2):
        for t in inputs:
            outs = [nan(), nan()]
            outs[k] = t
            with pytest.raises(_lib.MecanoHipError):
                hm.aba_jvp(*inputs, GRAVITY, None, out=tuple(outs))
            torch.cuda.synchronize()
            assert torch.isnan(outs[1 - k]).all()
    both = nan()
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_jvp(*inputs, GRAVITY, None, out=(both, both))
    torch.cuda.synchronize()
    assert torch.isnan(both).all()
    assert all(torch.equal(a, b) for a, b in zip((q, qd, qdd) + ds, before))
    modes = [0] * n
    modes[2] = 1
    hm.set_joint_source_modes(modes)
    out = nan()
    for method, x3, o in ((hm.rnea_jvp, qdd, out), (hm.aba_jvp, tau, (None, out))):
        with pytest.raises(_lib.MecanoHipError):
            method(q, qd, x3, *ds, GRAVITY, None, out=o)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    hm.set_joint_source_modes(None)
