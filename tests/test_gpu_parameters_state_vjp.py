"""mh_rnea_parameters_state_vjp_* / mh_aba_parameters_state_vjp_* and the autograd functions on the device against the CPU checker
(tests/parameters_state_vjp_check.py: row r's state gradients from tests/dynamics_vjp_check.py on the description with row r's inertias,
row r's parameter gradient from tests/parameters_vjp_check.py; pinned by tests/test_parameters_state_vjp_cpu.py) and against the device's
own neighbours at shared parameters (rnea_vjp, aba_vjp, rnea_parameters_vjp, aba_parameters_vjp).

Bounds, per configuration, the project's own.  State gradients as in tests/test_gpu_dynamics_vjp.py: |u|_1 TOL max(1, |D_ref|_inf) for
the inverse form (H(pi_r) in place of D for gqdd), |w|_1 8 sqrt(8 * 3 n) cond_inf(H(pi_r)) u max(1, |D_ref|_inf) for the forward form,
its qdd through helpers.close_aba.  gpi as in tests/test_gpu_parameters_vjp.py: the same with |Y|_inf / |H^-1 Y|_inf for the scale and
the factor chi = max over the bodies of max(1, m, 1 + |c|_1) of the chain rule.  fp32: helpers.f32_forward_tol(3 n) in place of TOL and
u = 2^-24, the checker fed the fp32-rounded inputs.  Every check records achieved / bound (helpers.record_parity)."""
import functools
import itertools

import numpy as np
import pytest

import helpers as hp
import inertial_parameters_check as ipc
import parameters_state_vjp_check as sc
from helpers import DistinctRows, check_bad_outputs, close_aba, f32_aba_forward_factor, f32_forward_tol, group_cover, poisoned, record_parity
from mecano_amd import random_tools as rt
from test_gravity_gradient_cpu import GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu

TOL = 1.0e-10
AOS, SOA = 0, 1
U64, U32 = 2.0 ** -53, 2.0 ** -24
TREE_ROWS = np.array([0, 1, 31, 63, 64, 69])  # (the checker takes seconds per row of the 128-body tree)
POOL = 13  # parameter sets of the batch-shape tests: row r takes set r % 13, a period that divides no group of 64
INV_NAMES, FWD_NAMES = ("gq", "gqd", "gqdd", "gpi"), ("qdd", "gq", "gqd", "gtau", "gpi")


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def model_of(desc):
    from mecano_amd.engine import HipModel
    return HipModel(desc)


def dev(torch, x, dtype=None):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def soa(x):
    """[B, ...] -> [prod(...), B] contiguous"""
    return None if x is None else x.reshape(x.shape[0], -1).t().contiguous()


def host(t, layout):
    """The output as an AoS-shaped fp64 array, [B, columns]."""
    return None if t is None else (t.t() if layout == SOA else t.reshape(t.shape[0], -1)).cpu().numpy().astype(np.float64)


def state(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)


def cotangent(B, nv, seed=8):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, nv))


def parameters(desc, B, seed=4):
    """[B, n, 10]: a different physical parameter set in every row."""
    return ipc.physical_parameter_sets(desc, np.random.default_rng(seed), B)


def call(torch, method, arrays, f, layout=AOS, dtype=None, gravity=GRAVITY, **kw):
    """hm.rnea_parameters_state_vjp / hm.aba_parameters_state_vjp on host arrays (q, qd, qdd | tau, pi, u | w): the outputs as AoS-shaped
    fp64 arrays [B, columns] (gpi: [B, 10 n]); None where the output was not asked for."""
    B = arrays[0].shape[0]
    args = [dev(torch, None if x is None else np.asarray(x).reshape(B, -1), dtype) for x in arrays] + [dev(torch, f, dtype)]
    if layout == SOA:
        args = [soa(x) for x in args]
    out = method(*args[:5], gravity, args[5], layout, **kw)
    torch.cuda.synchronize()
    return tuple(host(t, layout) for t in out)


def held(got, ref, bound, label, rows=None):
    """|got - ref|_inf <= bound per configuration; the worst achieved / bound goes to the parity log."""
    ref = ref.reshape(len(ref), -1)
    assert got.shape == ref.shape, label
    rows = np.arange(len(ref)) if rows is None else rows
    assert not np.isnan(got[rows]).any(), label
    ratio = float((np.abs(got - ref).max(axis=1)[rows] / bound[rows]).max())
    record_parity(ratio, 1.0, label + " achieved / bound")
    print(f"{label}: achieved / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{label}: achieved / bound = {ratio:.3e}"
    return ratio


def inverse_bounds(u, scales, tol=TOL):
    """Bounds of (gq, gqd, gqdd, gpi) from the checker's scales (|dtau/dq|, |dtau/dqd|, |H|, |Y|, chi, cond)."""
    l1 = np.abs(u).sum(axis=1)
    return [l1 * tol * np.maximum(1.0, s) for s in scales[:3]] + [l1 * tol * np.maximum(1.0, scales[3]) * scales[4]]


def forward_bounds(w, scales, n_joints, unit):
    """Bounds of (gq, gqd, gtau, gpi) from the checker's scales (|dqdd/dq|, |dqdd/dqd|, |H^-1|, |H^-1 Y|, chi, cond)."""
    base = np.abs(w).sum(axis=1) * f32_aba_forward_factor(3 * n_joints) * scales[5] * unit
    return [base * np.maximum(1.0, s) for s in scales[:3]] + [base * np.maximum(1.0, scales[3]) * scales[4]]


def hold_inverse(got, ref, u, label, tol=TOL, rows=None):
    *grads, scales = ref
    for g, r, b, name in zip(got, grads, inverse_bounds(u, scales, tol), INV_NAMES):
        if g is not None:
            held(g, r, b, f"{label} {name}", rows)


def hold_forward(got, ref, w, n_joints, label, unit=U64, rows=None):
    qdd_ref, *grads, scales = ref
    at = np.arange(len(qdd_ref)) if rows is None else rows
    if got[0] is not None:
        close_aba(got[0][at], qdd_ref[at], None, n_joints, unit, label=f"{label} qdd", conds=scales[5][at])
    for g, r, b, name in zip(got[1:], grads, forward_bounds(w, scales, n_joints, unit), FWD_NAMES[1:]):
        if g is not None:
            held(g, r, b, f"{label} forward {name}", rows)


# The inputs and references of a case are computed once and shared by the layouts (and never written to).  fp32: the checker sees what
# the device holds.  Rows 0 and 1 hold the same state and cotangents and different parameters.
def case_of(name):
    return sc.floating_tree7() if name == "n3_floating_tree7" else make_case(name)


@functools.lru_cache(maxsize=None)
def case_inputs(case, B=65, single=False, own=False):
    sys_, desc = case_of(case)
    q, qd, qdd, tau = state(sys_, B)
    pi = np.broadcast_to(ipc.parameters_of(desc), (B, desc.n_joints, 10)).copy() if own else parameters(desc, B)
    u, w = cotangent(B, desc.nv), cotangent(B, desc.nv, 9)
    f = random_wrenches(np.random.default_rng(21), B, desc.n_joints)
    for x in (q, qd, qdd, tau, u, w, f):
        x[1] = x[0]
    arrays = (q, qd, qdd, tau, pi, u, w, f)
    if single:
        arrays = tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in arrays)
    return (desc,) + arrays


@functools.lru_cache(maxsize=None)
def inverse_reference(case, wrenches, single=False, own=False):
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case, single=single, own=own)
    return sc.rnea_parameters_state_vjp(desc, q, qd, qdd, pi, u, GRAVITY, f if wrenches else None)


@functools.lru_cache(maxsize=None)
def forward_reference(case, wrenches, single=False, own=False):
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case, single=single, own=own)
    return sc.aba_parameters_state_vjp(desc, q, qd, tau, pi, w, GRAVITY, f if wrenches else None)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("wrenches", [False, True])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_fp64_matches_checker(torch_cuda, case, layout, wrenches):
    """B = 65: one full wave plus a ragged one, small enough that several waves share a group (parts > 1); a different physical
    parameter set in every row; all four / five outputs.  Rows 0 and 1 differ in their parameters only and must differ in gq: a kernel
    that read the model's constant inertia (or a neighbour's pi) fails either this or the bound."""
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case)
    hm, fe = model_of(desc), f if wrenches else None
    got = call(torch_cuda, hm.rnea_parameters_state_vjp, (q, qd, qdd, pi, u), fe, layout)
    hold_inverse(got, inverse_reference(case, wrenches), u, f"{case} layout {layout}")
    assert np.abs(got[0][0] - got[0][1]).max() > 1e-3 and np.abs(got[2][0] - got[2][1]).max() > 1e-3
    got = call(torch_cuda, hm.aba_parameters_state_vjp, (q, qd, tau, pi, w), fe, layout)
    hold_forward(got, forward_reference(case, wrenches), w, desc.n_joints, f"{case} layout {layout}")
    assert np.abs(got[1][0] - got[1][1]).max() > 1e-3


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_reduces_to_the_shared_parameter_calls(torch_cuda, case, layout):
    """Every row at inertial_parameters(): the outputs agree with hm.rnea_vjp / hm.aba_vjp and with hm.rnea_parameters_vjp /
    hm.aba_parameters_vjp within the bounds both are held to against the checker (not bit for bit: the device maps the ten numbers to its
    record), and with the checker at the description itself."""
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case, own=True)
    hm = model_of(desc)
    assert np.array_equal(pi[0], hm.inertial_parameters())
    put = lambda x: dev(torch, x.reshape(len(x), -1)) if layout == AOS else soa(dev(torch, x.reshape(len(x), -1)))
    Q, QD, QDD, TAU, PI, U, W, F = (put(x) for x in (q, qd, qdd, tau, pi, u, w, f))
    ref_i, ref_f = inverse_reference(case, True, own=True), forward_reference(case, True, own=True)
    got = call(torch, hm.rnea_parameters_state_vjp, (q, qd, qdd, pi, u), f, layout)
    hold_inverse(got, ref_i, u, f"{case} own parameters layout {layout}")
    shared = [host(t, layout) for t in hm.rnea_vjp(Q, QD, QDD, U, GRAVITY, F, layout)] + [host(hm.rnea_parameters_vjp(Q, QD, QDD, PI, U, GRAVITY, layout), layout)]
    for g, r, b, name in zip(got, shared, inverse_bounds(u, ref_i[-1]), INV_NAMES):
        held(g, r, b, f"{case} {name} against the shared-parameter call, layout {layout}")
    got = call(torch, hm.aba_parameters_state_vjp, (q, qd, tau, pi, w), f, layout)
    hold_forward(got, ref_f, w, desc.n_joints, f"{case} own parameters layout {layout}")
    a = [host(t, layout) for t in hm.aba_vjp(Q, QD, TAU, W, GRAVITY, F, layout)]
    p = [host(t, layout) for t in hm.aba_parameters_vjp(Q, QD, TAU, PI, W, GRAVITY, F, layout)]
    close_aba(got[0], a[0], None, desc.n_joints, U64, label="qdd against aba_vjp", conds=ref_f[-1][5])
    for g, r, b, name in zip(got[1:], a[1:] + [p[2]], forward_bounds(w, ref_f[-1], desc.n_joints, U64), FWD_NAMES[1:]):
        held(g, r, b, f"{case} forward {name} against the shared-parameter call, layout {layout}")
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_fp32_matches_checker(torch_cuda, layout):
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs("humanoid30", single=True)
    hm, n = model_of(desc), desc.n_joints
    got = call(torch, hm.rnea_parameters_state_vjp, (q, qd, qdd, pi, u), f, layout, dtype=torch.float32)
    hold_inverse(got, inverse_reference("humanoid30", True, single=True), u, f"fp32 layout {layout}", tol=f32_forward_tol(3 * n))
    got = call(torch, hm.aba_parameters_state_vjp, (q, qd, tau, pi, w), f, layout, dtype=torch.float32)
    hold_forward(got, forward_reference("humanoid30", True, single=True), w, n, f"fp32 layout {layout}", unit=U32)


def test_tree128_rows(torch_cuda):
    """The committed 128-body benchmark tree, nv = 323, fp64 AoS, B = 70: both calls on the rows TREE_ROWS, a different parameter set in
    each; every row free of NaN."""
    sys_ = rt.committedBenchmarkSystems()["tree128"]
    desc = sys_.toModelDesc()
    hm, B, n = model_of(desc), 70, desc.n_joints
    q, qd, qdd, tau = state(sys_, B)
    pool = parameters(desc, len(TREE_ROWS))
    pi = pool[np.arange(B) % len(TREE_ROWS)]
    pi[TREE_ROWS] = pool  # a different set in every checked row
    u = cotangent(B, desc.nv)
    f = random_wrenches(np.random.default_rng(22), B, n)
    got = call(torch_cuda, hm.rnea_parameters_state_vjp, (q, qd, qdd, pi, u), f)
    assert all(np.isfinite(g).all() for g in got)
    hold_inverse(got, sc.rnea_parameters_state_vjp(desc, q, qd, qdd, pi, u, GRAVITY, f, rows=TREE_ROWS), u, "tree128", rows=TREE_ROWS)
    got = call(torch_cuda, hm.aba_parameters_state_vjp, (q, qd, tau, pi, u), f)
    assert all(np.isfinite(g).all() for g in got)
    hold_forward(got, sc.aba_parameters_state_vjp(desc, q, qd, tau, pi, u, GRAVITY, f, rows=TREE_ROWS), u, n, "tree128", rows=TREE_ROWS)


# ------------------------------------------------------------------------------------------------ cover of batches
def _cover_case(torch, case, B, grid, layout, with_f, forward):
    """B distinct states, row r with parameter set r % POOL, poisoned outputs with a guard row behind them; the rows of
    helpers.group_cover -- every row group -- against the checker."""
    sys_, desc = make_case(case)
    hm, n, nv = model_of(desc), desc.n_joints, desc.nv
    rows = DistinctRows(sys_, 256, seed=29)
    q, qd, qdd, tau = rows.device(torch, B)
    idx = group_cover(B, grid)
    pool = parameters(desc, POOL, seed=16)
    u_host = cotangent(64, nv, 13)
    f_host = random_wrenches(np.random.default_rng(24), 64, n) if with_f else None
    r = torch.arange(B, device="cuda")
    pi = dev(torch, pool.reshape(POOL, -1))[r % POOL].contiguous()
    u = dev(torch, u_host)[r % 64].contiguous()
    f = dev(torch, f_host)[r % 64].contiguous() if with_f else None
    shapes = [(nv,)] * (5 if forward else 4)
    shapes[-1] = (10 * n,)
    bufs = [poisoned(torch, B, s, torch.float64) if layout == AOS else poisoned(torch, s[0], (B,), torch.float64) for s in shapes]
    x3 = tau if forward else qdd
    args = (q, qd, x3, pi, u, GRAVITY, f) if layout == AOS else (soa(q), soa(qd), soa(x3), soa(pi), soa(u), GRAVITY, soa(f))
    (hm.aba_parameters_state_vjp if forward else hm.rnea_parameters_state_vjp)(*args, layout, out=tuple(b[0] for b in bufs))
    torch.cuda.synchronize()
    take = torch.as_tensor(idx, device="cuda")
    got = []
    for k, (o, g) in enumerate(bufs):
        assert torch.isnan(g).all(), f"output {k}: wrote past the last row"
        assert not torch.isnan(o).any(), f"output {k}: entries left unwritten (NaN)"
        got.append((o if layout == AOS else o.t())[take].cpu().numpy())
    qi, qdi, qddi, taui = rows.rows(idx)
    ui, fi, pii = u_host[idx % 64], None if f_host is None else f_host[idx % 64], pool[idx % POOL]
    label = f"{case} B {B} layout {layout}"
    if forward:
        hold_forward(got, sc.aba_parameters_state_vjp(desc, qi, qdi, taui, pii, ui, GRAVITY, fi), ui, n, label)
    else:
        hold_inverse(got, sc.rnea_parameters_state_vjp(desc, qi, qdi, qddi, pii, ui, GRAVITY, fi), ui, label)


@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("B", [1, 63, 64, 257])
def test_ragged_and_full_batches_cover_every_row_group(torch_cuda, B, layout, forward):
    _cover_case(torch_cuda, "arm7", B, None, layout, with_f=(B % 2 == 1), forward=forward)


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the grid holds (8 per CU), plus a ragged last group: every lane loops over several groups of 64, one
    wave per group (parts = 1).  The forward form is two launches of mh_aba_parameters_*, whose own tests cover their row groups, and this
    kernel."""
    cus = int(torch_cuda.cuda.get_device_properties(0).multi_processor_count)
    _cover_case(torch_cuda, "arm7", 2 * 8 * cus * 64 + 64 + 37, 8 * cus, layout, with_f=True, forward=False)


# ------------------------------------------------------------------------------------------------ output selection
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_each_output_null_in_turn_leaves_the_others_bit_for_bit(torch_cuda, layout):
    """humanoid30, B = 64 * 5 + 3, wrenches: each output None in turn, gpi included (and qdd_out of the forward form) -- the others have
    the bits of the call that asks for everything; all gradients None is refused."""
    from mecano_amd import _lib
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, n, nv = model_of(desc), 64 * 5 + 3, desc.n_joints, desc.nv
    q, qd, qdd, tau = state(sys_, B)
    pi, u = parameters(desc, POOL)[np.arange(B) % POOL], cotangent(B, nv)
    f = random_wrenches(np.random.default_rng(27), B, n)
    put = lambda x: dev(torch, x.reshape(len(x), -1)) if layout == AOS else soa(dev(torch, x.reshape(len(x), -1)))
    Q, QD, QDD, TAU, PI, U, F = (put(x) for x in (q, qd, qdd, tau, pi, u, f))
    for method, x3, count in ((hm.rnea_parameters_state_vjp, QDD, 4), (hm.aba_parameters_state_vjp, TAU, 5)):
        full = method(Q, QD, x3, PI, U, GRAVITY, F, layout)
        assert all(torch.isfinite(t).all() for t in full)
        for skip in range(count):
            outs = [None if k == skip else torch.full_like(t, float("nan")) for k, t in enumerate(full)]
            res = method(Q, QD, x3, PI, U, GRAVITY, F, layout, out=tuple(outs))
            torch.cuda.synchronize()
            assert res[skip] is None
            assert all(torch.equal(a, b) for k, (a, b) in enumerate(zip(res, full)) if k != skip), (method.__name__, skip)
        with pytest.raises(_lib.MecanoHipError):
            method(Q, QD, x3, PI, U, GRAVITY, F, layout, out=(torch.empty_like(full[0]),) + (None,) * 4 if count == 5 else (None,) * 4)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case,B", [("arm7", 1), ("arm7", 65), ("humanoid30", 197)])
def test_forward_outputs_null_together_leave_the_others_bit_for_bit(torch_cuda, case, B, layout, dtype_name):
    """The forward form with several outputs None at once: gtau alone (no qdd is needed: the first forward-dynamics launch is skipped),
    qdd and gtau (no adjoint launch), gpi alone and gq, gqd, gpi (qdd and H^-1 w both in the context's scratch) -- what is asked for has
    the bits of the call that asks for everything."""
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc = make_case(case)
    hm, n, nv = model_of(desc), desc.n_joints, desc.nv
    q, qd, _, tau = state(sys_, B)
    pi, w = parameters(desc, POOL)[np.arange(B) % POOL], cotangent(B, nv, 9)
    f = random_wrenches(np.random.default_rng(27), B, n)
    put = lambda x: dev(torch, x.reshape(len(x), -1), dtype) if layout == AOS else soa(dev(torch, x.reshape(len(x), -1), dtype))
    Q, QD, TAU, PI, W, F = (put(x) for x in (q, qd, tau, pi, w, f))
    full = hm.aba_parameters_state_vjp(Q, QD, TAU, PI, W, GRAVITY, F, layout)
    assert all(torch.isfinite(t).all() for t in full)
    for keep in ((3,), (0, 3), (4,), (1, 2, 4)):  # of (qdd, gq, gqd, gtau, gpi)
        outs = [torch.full_like(t, float("nan")) if k in keep else None for k, t in enumerate(full)]
        res = hm.aba_parameters_state_vjp(Q, QD, TAU, PI, W, GRAVITY, F, layout, out=tuple(outs))
        torch.cuda.synchronize()
        assert all((r is None) if k not in keep else torch.equal(r, full[k]) for k, r in enumerate(res)), keep


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case,B", [("arm7", 65), ("humanoid30", 197)])
def test_forward_form_turns_both_switches_on(torch_cuda, case, B, layout, dtype_name):
    """mh_aba_parameters_state_vjp_* handed consider_coriolis = 0 and consider_accelerations = 0 through the C ABI (the engine never
    does): the per-row form runs forward dynamics and the adjoint sweep with both switches on whatever the caller sets -- every output
    has the bits of the engine's call."""
    import ctypes

    from mecano_amd import _lib
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc = make_case(case)
    hm, n, nv = model_of(desc), desc.n_joints, desc.nv
    q, qd, _, tau = state(sys_, B)
    pi, w = parameters(desc, POOL)[np.arange(B) % POOL], cotangent(B, nv, 9)
    f = random_wrenches(np.random.default_rng(27), B, n)
    put = lambda x: dev(torch, x.reshape(len(x), -1), dtype) if layout == AOS else soa(dev(torch, x.reshape(len(x), -1), dtype))
    Q, QD, TAU, PI, W, F = (put(x) for x in (q, qd, tau, pi, w, f))
    full = hm.aba_parameters_state_vjp(Q, QD, TAU, PI, W, GRAVITY, F, layout)
    outs = [torch.full_like(t, float("nan")) for t in full]
    g, ra = hm._root(GRAVITY)
    opts = hm._options(layout, False, False, torch.cuda.current_stream().cuda_stream, root_acceleration=ra)
    _lib.check(getattr(_lib.load(), "mh_aba_parameters_state_vjp_" + ("f64" if dtype_name == "float64" else "f32"))(
        hm._h, B, Q.data_ptr(), QD.data_ptr(), TAU.data_ptr(), PI.data_ptr(), g, F.data_ptr(), W.data_ptr(), ctypes.byref(opts),
        *(o.data_ptr() for o in outs)))
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in full) and full[2].any()
    assert all(torch.equal(a, b) for a, b in zip(outs, full))


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_exact_zeros(torch_cuda, layout):
    """u = 0 gives exact zeros in every output, gpi included (w = 0 in the forward form); consider_coriolis=False gives exact zeros in
    gqd, needs no qd and has the bits of qd = 0; consider_accelerations=False those of qdd = 0."""
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs("humanoid30")
    hm, z = model_of(desc), np.zeros_like(u)
    assert not any(g.any() for g in call(torch, hm.rnea_parameters_state_vjp, (q, qd, qdd, pi, z), f, layout))
    assert not any(g.any() for g in call(torch, hm.aba_parameters_state_vjp, (q, qd, tau, pi, z), f, layout)[1:])
    off = call(torch, hm.rnea_parameters_state_vjp, (q, None, qdd, pi, u), f, layout, consider_coriolis=False)
    ref = call(torch, hm.rnea_parameters_state_vjp, (q, z, qdd, pi, u), f, layout)
    assert all(np.array_equal(a, b) for a, b in zip(off, ref)) and not off[1].any() and off[0].any() and off[3].any()
    off = call(torch, hm.rnea_parameters_state_vjp, (q, qd, None, pi, u), f, layout, consider_accelerations=False)
    ref = call(torch, hm.rnea_parameters_state_vjp, (q, qd, z, pi, u), f, layout)
    assert all(np.array_equal(a, b) for a, b in zip(off, ref))


def test_unowned_dof_indices_get_zeros(torch_cuda):
    """A custom index map with two DoF / configuration indices no joint owns, every output in a poisoned buffer with a guard row behind
    it: zeros there, the default map's values elsewhere (the same kernel on the same numbers: bit for bit in the inverse form)."""
    torch = torch_cuda
    sys_, d0 = make_case("onedof_tree")
    B, nv, n = 70, d0.nv, d0.n_joints
    q, qd, qdd, tau = state(sys_, B)
    u, pi = cotangent(B, nv), parameters(d0, B)
    place = np.array([k + (k >= 3) + (k >= 7) for k in range(nv)])  # indices 3 and 8 of the wide map stay free
    free = np.setdiff1d(np.arange(nv + 2), place)
    d1 = sys_.toModelDesc()
    d1.dof_indices = place[np.asarray(d0.dof_indices)].astype(np.int32)
    d1.cfg_indices = place[np.asarray(d0.cfg_indices)].astype(np.int32)
    d1.nv = d1.nq = nv + 2
    wide = lambda x: np.ascontiguousarray(np.insert(np.insert(x, 3, 0.25, axis=1), 8, -0.5, axis=1))
    h0, h1 = model_of(d0), model_of(d1)
    base_i = call(torch, h0.rnea_parameters_state_vjp, (q, qd, qdd, pi, u), None)
    ref_f = sc.aba_parameters_state_vjp(d0, q, qd, tau, pi, u, GRAVITY)
    for layout in (AOS, SOA):
        def buffers(count):
            shapes = [(nv + 2,)] * (count - 1) + [(10 * n,)]
            return [poisoned(torch, B, s, torch.float64) if layout == AOS else poisoned(torch, s[0], (B,), torch.float64) for s in shapes]
        bi, bf = buffers(4), buffers(5)
        got_i = call(torch, h1.rnea_parameters_state_vjp, (wide(q), wide(qd), wide(qdd), pi, wide(u)), None, layout, out=tuple(b[0] for b in bi))
        got_f = call(torch, h1.aba_parameters_state_vjp, (wide(q), wide(qd), wide(tau), pi, wide(u)), None, layout, out=tuple(b[0] for b in bf))
        assert all(torch.isnan(g).all() for _, g in bi + bf), "wrote past an output"
        for k, g in enumerate(got_i):
            assert not np.isnan(g).any()
            if k < 3:
                assert not g[:, free].any(), f"output {k}"
                g = g[:, place]
            assert np.array_equal(g, base_i[k]), f"output {k}"
        # (qdd_out is what aba_parameters writes: as with aba, entries no joint owns are left alone)
        assert np.isnan(got_f[0][:, free]).all() and not np.isnan(got_f[0][:, place]).any()
        assert not any(np.isnan(g).any() for g in got_f[1:]) and not any(g[:, free].any() for g in got_f[1:4])
        hold_forward([g[:, place] for g in got_f[:4]] + [got_f[4]], ref_f, u, n, f"wide map layout {layout}")


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_a_bad_row_stays_alone(torch_cuda, layout):
    """One row whose leaf body has no mass and no inertia (no physical inertia: the leaf's 1 / D is 1 / 0): non-finite values in that
    row's outputs of the forward form only, every other row bit for bit what the clean batch gives -- and the clean batch is within
    bound against the checker.  The call returns MH_OK."""
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs("arm7")
    hm, k = model_of(desc), 40
    keep = np.arange(len(q)) != k
    clean_i = call(torch, hm.rnea_parameters_state_vjp, (q, qd, qdd, pi, u), f, layout)
    clean_f = call(torch, hm.aba_parameters_state_vjp, (q, qd, tau, pi, w), f, layout)
    hold_inverse(clean_i, inverse_reference("arm7", True), u, f"clean batch layout {layout}")
    hold_forward(clean_f, forward_reference("arm7", True), w, desc.n_joints, f"clean batch layout {layout}")
    bad = pi.copy()
    leaf = [j for j in range(desc.n_joints) if j not in set(int(p) for p in desc.parent)][-1]
    bad[k, leaf] = 0.0
    got_i = call(torch, hm.rnea_parameters_state_vjp, (q, qd, qdd, bad, u), f, layout)
    got_f = call(torch, hm.aba_parameters_state_vjp, (q, qd, tau, bad, w), f, layout)
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(clean_i, got_i))
    assert all(np.array_equal(a[keep], b[keep]) and np.isfinite(b[keep]).all() for a, b in zip(clean_f, got_f))
    assert all(not np.isfinite(g[k]).all() for g in got_f)


# ------------------------------------------------------------------------------------------------ scattered index maps
@functools.lru_cache(maxsize=None)
def _scattered_reference(model, single):
    """States, parameters and cotangents in the identity description's index space and the checker's outputs on them: once per model and
    precision, shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    B, np_dt = 70, (np.float32 if single else np.float64)
    q, qd, qdd, tau = DistinctRows(sys_, 16, seed=61).rows(np.arange(B), np_dt)
    rnd = lambda x: np.asarray(x, dtype=np_dt).astype(np.float64)
    pi, u, w = rnd(parameters(d0, B, 62)), rnd(cotangent(B, d0.nv, 63)), rnd(cotangent(B, d0.nv, 64))
    f = rnd(random_wrenches(np.random.default_rng(65), B, d0.n_joints))
    ref_i = sc.rnea_parameters_state_vjp(d0, q, qd, qdd, pi, u, GRAVITY, f)
    ref_f = sc.aba_parameters_state_vjp(d0, q, qd, tau, pi, w, GRAVITY, f)
    assert ref_f[-1][5].max() < 1.0e8  # cond_inf(H(pi_r)) of every row
    return (q, qd, qdd, tau, pi, u, w, f), ref_i, ref_f


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """Both calls on a description whose maps send every DoF and every configuration entry somewhere else (with holes: two indices of each
    space owned by no joint, holding 7.0 in every input, the cotangent included), a different parameter set in every row, against the
    checker on the IDENTITY description: the state gradients come back through the DoF map and meet hold_inverse's / hold_forward's
    bounds, gpi follows the listing order of the joints and does NOT move; the gradients at unowned indices are exact zeros, the guard
    rows stay poisoned; each output asked for alone (the others NULL) meets the same bound; read without moving them back the state
    gradients miss the reference by more than 1e-3."""
    torch = torch_cuda
    single = dtype_name == "float32"
    dtype, unit = getattr(torch, dtype_name), (U32 if single else U64)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, n = hp.scattered_model(d, model), 70, d.nv, d0.n_joints
    (q, qd, qdd, tau, pi, u, w, f), ref_i, ref_f = _scattered_reference(model, single)
    is_soa = layout == SOA
    put = lambda x: soa(dev(torch, x.reshape(B, -1), dtype)) if is_soa else dev(torch, x.reshape(B, -1), dtype)
    tq = put(hp.to_q(q, pq, d.nq))
    tqd, tqdd, ttau, tu, tw = (put(hp.to_v(x, pv, nv)) for x in (qd, qdd, tau, u, w))
    tpi, tf = put(pi), put(f)

    def run(issue, shapes, want):
        """[(moved back, unowned entries, as the device wrote it)] of the outputs `want`; gpi ([B, 10 n]) is not moved"""
        outs, guards = hp.poisoned_set(torch, B, shapes, dtype, is_soa)
        outs = [o if k in want else None for k, o in enumerate(outs)]
        issue(tuple(outs))
        torch.cuda.synchronize()
        hp.guards_intact([g for k, g in enumerate(guards) if k in want])
        res = []
        for o, s in zip(outs, shapes):
            raw = None if o is None else hp.rows_of(o, B, s, is_soa)
            res.append(None if o is None else ((raw, raw[:, :0], raw) if s != (nv,) else hp.from_v(raw, pv) + (raw,)))
        return res

    def check(got, names, hold):
        for k, g in enumerate(got):
            if g is not None and names[k] != "qdd":  # (qdd is no gradient: its unowned entries are not written)
                assert not g[1].any(), names[k]  # exact zeros at unowned indices, and written
        hold([None if g is None else g[0] for g in got])

    inverse = lambda out: hm.rnea_parameters_state_vjp(tq, tqd, tqdd, tpi, tu, GRAVITY, tf, layout, out=out)
    forward = lambda out: hm.aba_parameters_state_vjp(tq, tqd, ttau, tpi, tw, GRAVITY, tf, layout, out=out)
    tol = f32_forward_tol(3 * n) if single else TOL
    shapes = [(nv,)] * 3 + [(10 * n,)]
    got = run(inverse, shapes, (0, 1, 2, 3))
    check(got, INV_NAMES, lambda g: hold_inverse(g, ref_i, u, "scattered", tol))
    for k in range(4):
        check(run(inverse, shapes, (k,)), INV_NAMES, lambda g: hold_inverse(g, ref_i, u, f"scattered, {INV_NAMES[k]} alone", tol))
    for k in range(3):
        hp.assert_misses(hp.keep_order(got[k][2], pv), ref_i[k], INV_NAMES[k])
    shapes = [(nv,)] * 4 + [(10 * n,)]
    got = run(forward, shapes, (0, 1, 2, 3, 4))
    check(got, FWD_NAMES, lambda g: hold_forward(g, ref_f, w, n, "scattered", unit))
    for k in range(1, 5):
        check(run(forward, shapes, (k,)), FWD_NAMES, lambda g: hold_forward(g, ref_f, w, n, f"scattered, {FWD_NAMES[k]} alone", unit))
    for k in range(4):
        hp.assert_misses(hp.keep_order(got[k][2], pv), ref_f[k], "forward " + FWD_NAMES[k])


# ------------------------------------------------------------------------------------------------ plumbing
def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() and a first call both calls are
    captured into a graph (they allocate nothing) and the replay gives the bits of the direct call, also on new pi and w."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = model_of(desc), 1000
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    w = dev(torch, cotangent(B, desc.nv, 9))
    pool = parameters(desc, 50)
    pi = dev(torch, pool[np.arange(B) % 50].reshape(B, -1))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    ref_i = hm.rnea_parameters_state_vjp(q, qd, qdd, pi, w, GRAVITY, f)
    ref_f = hm.aba_parameters_state_vjp(q, qd, tau, pi, w, GRAVITY, f)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    out_i = tuple(torch.empty_like(t) for t in ref_i)
    out_f = (None, torch.empty_like(ref_f[1]), torch.empty_like(ref_f[2]), None, torch.empty_like(ref_f[4]))  # qdd, mu: the context's scratch
    mine = out_i + (out_f[1], out_f[2], out_f[4])
    same = lambda ri, rf: all(torch.equal(a, b) for a, b in zip(mine, tuple(ri) + (rf[1], rf[2], rf[4])))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view.rnea_parameters_state_vjp(q, qd, qdd, pi, w, GRAVITY, f, out=out_i)
        view.aba_parameters_state_vjp(q, qd, tau, pi, w, GRAVITY, f, out=out_f)
        view.check(s.cuda_stream)
        assert same(ref_i, ref_f)
        for t in mine:
            t.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            view.rnea_parameters_state_vjp(q, qd, qdd, pi, w, GRAVITY, f, out=out_i)
            view.aba_parameters_state_vjp(q, qd, tau, pi, w, GRAVITY, f, out=out_f)
    torch.cuda.synchronize()
    assert not any(t.any() for t in mine)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert same(ref_i, ref_f)
    pi2, w2 = dev(torch, pool[(np.arange(B) + 7) % 50].reshape(B, -1)), dev(torch, cotangent(B, desc.nv, 14))
    ref_i2 = hm.rnea_parameters_state_vjp(q, qd, qdd, pi2, w2, GRAVITY, f)
    ref_f2 = hm.aba_parameters_state_vjp(q, qd, tau, pi2, w2, GRAVITY, f)
    pi.copy_(pi2), w.copy_(w2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same(ref_i2, ref_f2) and not torch.equal(ref_f2[4], ref_f[4])
    view.close()


def test_wrong_shapes_overlaps_and_source_joints_are_refused(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = model_of(desc), 10, desc.nv, desc.n_joints
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    u, pi = dev(torch, cotangent(B, nv)), dev(torch, parameters(desc, B))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    calls = ((hm.rnea_parameters_state_vjp, qdd, 4), (hm.aba_parameters_state_vjp, tau, 5))
    for method, x3, count in calls:
        for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(B, n, 5)):
            with pytest.raises(_lib.MecanoHipError):
                method(q, qd, x3, pi, u, GRAVITY, bad_f)
        for bad_pi in (None, pi[:, :-1].contiguous(), z(B + 1, n, 10), z(n * 10, B)):
            with pytest.raises(_lib.MecanoHipError):
                method(q, qd, x3, bad_pi, u, GRAVITY)
        with pytest.raises(_lib.MecanoHipError):
            method(q, qd, x3, pi, z(B, nv + 1), GRAVITY)
        with pytest.raises(_lib.MecanoHipError):
            method(q, qd, x3, pi, u, GRAVITY, out=(None,) * count)
        with pytest.raises(_lib.MecanoHipError):
            method(q, qd, x3, pi, u, GRAVITY, out=(None,) * (count - 1))  # a tuple of the wrong length
        shapes = [(B, nv)] * (count - 1) + [(B, n, 10)]
        check_bad_outputs(torch, shapes, lambda out, m=method, x=x3: m(q, qd, x, pi, u, GRAVITY, None, out=out))
        # every forbidden overlap: an output on an input of its size (pi with gpi, the cotangent with gq among them; q has nq = nv
        # here), two outputs of one size on each other -- nothing is written
        nan = lambda shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        inputs = (q, qd, x3, u)
        before = [t.clone() for t in inputs + (pi,)]
        for k in range(count):
            for t in ((pi,) if k == count - 1 else inputs):
                outs = [nan(s) for s in shapes]
                outs[k] = t
                with pytest.raises(_lib.MecanoHipError):
                    method(q, qd, x3, pi, u, GRAVITY, None, out=tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for j, o in enumerate(outs) if j != k)
            for j in range(k if k < count - 1 else 0):
                outs = [nan(s) for s in shapes]
                outs[k] = outs[j]
                with pytest.raises(_lib.MecanoHipError):
                    method(q, qd, x3, pi, u, GRAVITY, None, out=tuple(outs))
                torch.cuda.synchronize()
                assert all(torch.isnan(o).all() for o in outs)
        assert all(torch.equal(a, b) for a, b in zip(inputs + (pi,), before))
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_parameters_state_vjp(q, qd, None, pi, u, GRAVITY)
    modes = [0] * n
    modes[2] = 1
    hm.set_joint_source_modes(modes)
    for method, x3, _ in calls:
        with pytest.raises(_lib.MecanoHipError):
            method(q, qd, x3, pi, u, GRAVITY)
    hm.set_joint_source_modes(None)


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_is_the_method_plus_the_pullback_for_every_subset_of_inputs(torch_cuda):
    """humanoid30 (floating root), B = 70, fp64: for every non-empty subset of (q, qd, qdd | tau, pi) that requires grad,
    torch.autograd.grad of sum(w * f(...)) is the method's output -- chart_pullback of gq for q -- bit for bit, the call is made with the
    other outputs None, and an input outside the subset gets no gradient; a second backward raises."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = model_of(desc), 70
    qh, qdh, qddh, tauh = state(sys_, B)
    pih, w = parameters(desc, B), dev(torch, cotangent(B, desc.nv, 9))
    f = dev(torch, random_wrenches(np.random.default_rng(28), B, desc.n_joints))
    for fn, name, x3h in ((mha.rnea_parameters_state, "rnea_parameters_state_vjp", qddh), (mha.aba_parameters_state, "aba_parameters_state_vjp", tauh)):
        vjp = getattr(hm, name)
        base = [dev(torch, x) for x in (qh, qdh, x3h, pih)]
        direct = list(vjp(*base, w, GRAVITY, f)[-4:])
        direct[0] = hm.chart_pullback(base[0], direct[0])
        for subset in itertools.chain.from_iterable(itertools.combinations(range(4), k) for k in range(1, 5)):
            args = [t.clone().requires_grad_(k in subset) for k, t in enumerate(base)]
            seen = {}
            setattr(hm, name, lambda *a, _v=vjp, **kw: (seen.update(out=kw["out"]), _v(*a, **kw))[1])
            try:
                loss = (w * fn(hm, *args, GRAVITY, f)).sum()
                got = torch.autograd.grad(loss, [args[k] for k in subset], create_graph=True)
            finally:
                delattr(hm, name)
            assert [t is not None for t in seen["out"]][-4:] == [k in subset for k in range(4)], subset
            assert all(torch.equal(g, direct[k]) for g, k in zip(got, subset)), (name, subset)
            unused = [args[k] for k in range(4) if k not in subset]
            assert all(not t.requires_grad for t in unused)
        with pytest.raises(RuntimeError):
            got[0].sum().backward()


def test_gradcheck_on_the_arm(torch_cuda):
    """torch.autograd.gradcheck of both functions jointly in (q, qd, qdd | tau, pi): arm7, fp64, B = 3, with the tolerances
    tests/test_gpu_parameters_vjp.py::test_gradcheck_on_the_arm derives for its central difference with eps = 1e-6: the efforts round to
    |tau| 2^-53 / eps, about 1e-8; the accelerations round to cond(H) 2^-53 |qdd| / eps, about 1e-6 at cond 1e2 and |qdd| 1e2, beside a
    truncation of eps^2 times the third derivative -- 1e-6 absolute + 1e-5 relative for the inverse dynamics and ten times that for the
    forward dynamics.  (The arm's coordinates are angles: raw coordinates and the chart coincide.)"""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B = model_of(desc), 3
    q, qd, qdd, tau = (dev(torch, x).requires_grad_() for x in state(sys_, B))
    pi = dev(torch, parameters(desc, B)).requires_grad_()
    assert torch.autograd.gradcheck(lambda *a: mha.rnea_parameters_state(hm, *a, GRAVITY), (q, qd, qdd, pi), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda *a: mha.aba_parameters_state(hm, *a, GRAVITY), (q, qd, tau, pi), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_step_parameters_rollout_against_a_central_difference(torch_cuda):
    """n3_floating_tree7 (SixDoF root), fp64, B = 5, three steps of dt = 0.01 through autograd.step_parameters with pi =
    shared.expand(B, n, 10): the gradient of a random linear loss on (q, qd) after the rollout with respect to the initial (q, qd) -- raw
    coordinates, quaternion included -- and to the shared pi, paired with one random direction, against the central difference of the
    loss along that direction with step h = 1e-5.  Derived as the tolerances of test_gradcheck_on_the_arm: the difference rounds to
    cond(H) 2^-53 |L| / h, about 1e-6 at cond 1e3 and |L| 1e2 (the loss sums B * (nq + nv) entries of size one), beside a truncation of
    h^2 / 6 times the third derivative, about 1e-8: the forward-dynamics tolerance, 1e-5 absolute + 1e-4 relative."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, desc = sc.floating_tree7()
    hm, B, n, steps, dt, h = model_of(desc), 5, desc.n_joints, 3, 0.01, 1.0e-5
    qh, qdh, _, tauh = state(sys_, B)
    rng = np.random.default_rng(33)
    q0, qd0, tau = dev(torch, qh), dev(torch, qdh), dev(torch, 0.1 * tauh)
    shared0 = dev(torch, parameters(desc, 1)[0])
    cq, cv = dev(torch, rng.uniform(-1, 1, qh.shape)), dev(torch, rng.uniform(-1, 1, qdh.shape))
    dq, dqd = dev(torch, rng.uniform(-1, 1, qh.shape)), dev(torch, rng.uniform(-1, 1, qdh.shape))
    dpi = shared0 * dev(torch, rng.uniform(-1, 1, (n, 10)))  # a relative change of every number

    def loss(q, qd, shared):
        pi = shared.expand(B, n, 10).contiguous()
        for _ in range(steps):
            q, qd = mha.step_parameters(hm, dt, q, qd, tau, pi, GRAVITY)
        return (cq * q).sum() + (cv * qd).sum()

    q, qd, shared = q0.clone().requires_grad_(), qd0.clone().requires_grad_(), shared0.clone().requires_grad_()
    gq, gqd, gpi = torch.autograd.grad(loss(q, qd, shared), (q, qd, shared))
    got = float((gq * dq).sum() + (gqd * dqd).sum() + (gpi * dpi).sum())
    with torch.no_grad():
        up = float(loss(q0 + h * dq, qd0 + h * dqd, shared0 + h * dpi))
        down = float(loss(q0 - h * dq, qd0 - h * dqd, shared0 - h * dpi))
    ref = (up - down) / (2.0 * h)
    bound = 1e-5 + 1e-4 * abs(ref)
    record_parity(abs(got - ref), bound, "rollout gradient against a central difference")
    print(f"rollout: directional derivative {got:.9e} against {ref:.9e}, |difference| / bound = {abs(got - ref) / bound:.3e}")
    assert gpi.shape == (n, 10) and float(gpi.abs().max()) > 0.0 and float(gq.abs().max()) > 0.0
    assert abs(got - ref) <= bound


# ------------------------------------------------------------------------------------------------ example
def test_the_trajectory_identification_example_lowers_its_loss(torch_cuda):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "identify_by_trajectory_error.py")
    spec = importlib.util.spec_from_file_location("identify_by_trajectory_error", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after = mod.main(samples=128, horizon=4, iterations=5)
    assert np.isfinite([before, after]).all() and after < before
