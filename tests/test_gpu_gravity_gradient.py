"""mh_gravity_gradient_f64 / _f32 on the device against the CPU checker (tests/gravity_gradient_check.py, pinned by
tests/test_gravity_gradient_cpu.py), through the C-ABI (HipModel.gravity_gradient is the ctypes call) and the calculator mirror."""
import ctypes
import functools

import numpy as np
import pytest

import gravity_gradient_check as gc
import helpers as hp
from helpers import DistinctRows, check_bad_outputs, check_cover, close, f32_forward_tol, group_cover, poisoned
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches, states, system_of

pytestmark = pytest.mark.gpu

TOL = 1.0e-10  # helpers.close default: relative to max(1, |ref|_inf)
AOS, SOA = 0, 1


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def soa(torch, x):
    """[B, ...] -> [prod(...), B] contiguous"""
    return None if x is None else x.reshape(x.shape[0], -1).t().contiguous()


def run(torch, hm, q, f, layout, dtype=None, out=None):
    """Device call on host arrays laid out as the call wants them; returns AoS-shaped numpy (tau [B, nv], grad [B, nv, nv])."""
    dq, df = dev(torch, q, dtype), dev(torch, f, dtype)
    if layout == SOA:
        dq, df = soa(torch, dq), soa(torch, df)
    tau, grad = hm.gravity_gradient(dq, GRAVITY, df, layout, out=out)
    torch.cuda.synchronize()
    B = q.shape[0]
    if layout == SOA:
        tau, grad = tau.t(), grad.t()
    return tau.cpu().numpy().astype(np.float64).reshape(B, hm.nv), grad.cpu().numpy().astype(np.float64).reshape(B, hm.nv, hm.nv)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("wrenches", ["none", "zero", "random"])
def test_fp64_matches_checker(torch_cuda, case, layout, wrenches):
    """Every model of the CPU pins, both layouts, without f_ext, with an all-zero f_ext and with random wrenches; 70 configurations: one
    full group of 64 and a ragged one, split over several waves per group (the column parts of small batches)."""
    from mecano_amd.engine import HipModel
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q = states(sys_, B)
    f = {"none": None, "zero": np.zeros((B, desc.n_joints, 6)),
         "random": random_wrenches(np.random.default_rng(21), B, desc.n_joints)}[wrenches]
    tau, grad = run(torch_cuda, hm, q, f, layout)
    tau_ref, grad_ref = gc.gravity_gradient(desc, q, GRAVITY, f)
    close(tau, tau_ref, TOL, label="tau")
    close(grad, grad_ref, TOL, label="grad")
    assert np.all(grad[:, ~gc.related(desc)] == 0.0)  # written, and exactly zero


@pytest.mark.parametrize("case", ["arm7", "humanoid30", "tree128"])
def test_fp32_matches_checker(torch_cuda, case):
    """fp32 on the arm, the humanoid and a 128-body random tree.  Bound, fixed before any run: an entry is an inward accumulation over a
    subtree of up to n bodies (first moment, external force) followed by a climb over up to n ancestors, each step a rotation and a sum --
    a recursion over at most 2 n bodies in helpers.f32_forward_tol's terms: 4 sqrt(8 * 2 n) 2^-24, relative to max(1, |ref|_inf).  The
    checker runs in fp64 on the fp32-rounded inputs."""
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    if case == "tree128":
        sys_ = system_of(rt.nextJointTree(np.random.default_rng(17), 128, ("revolute", "prismatic", "sixdof")))
        desc = sys_.toModelDesc()
    else:
        sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q = states(sys_, B).astype(np.float32)
    f = random_wrenches(np.random.default_rng(22), B, desc.n_joints).astype(np.float32)
    tol = f32_forward_tol(2 * desc.n_joints)
    rows = np.arange(B) if case != "tree128" else np.array([0, 1, 31, 63, 64, 69])  # (the checker takes seconds per row of that tree)
    for layout in (AOS, SOA):
        tau, grad = run(torch, hm, q, f, layout, torch.float32)
        tau_ref, grad_ref = gc.gravity_gradient(desc, q[rows].astype(np.float64), GRAVITY, f[rows].astype(np.float64))
        assert not np.isnan(tau).any() and not np.isnan(grad).any()
        close(tau[rows], tau_ref, tol, label=f"fp32 tau layout {layout}")
        close(grad[rows], grad_ref, tol, label=f"fp32 grad layout {layout}")


@pytest.mark.parametrize("case", CASES)
def test_tau_is_the_device_inverse_dynamics_with_both_switches_off(torch_cuda, case):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 200
    q = dev(torch, states(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(23), B, desc.n_joints))
    z = torch.zeros((B, desc.nv), dtype=torch.float64, device="cuda")
    for fe in (None, f):
        tau, _ = hm.gravity_gradient(q, GRAVITY, fe)
        ref = hm.rnea(q, z, z, GRAVITY, fe, consider_coriolis=False, consider_accelerations=False)
        close(tau.cpu().numpy(), ref.cpu().numpy(), TOL)


def _cover_case(torch, sys_, desc, B, grid, layout, with_f):
    """B distinct rows, poisoned outputs with a guard row behind them, every row group checked against the checker."""
    from mecano_amd.engine import HipModel
    hm = HipModel(desc)
    rows = DistinctRows(sys_, 256, seed=29)
    q = rows.device(torch, B)[0]
    idx = group_cover(B, grid)
    f_host = random_wrenches(np.random.default_rng(24), 64, desc.n_joints) if with_f else None
    f = None
    if with_f:  # row r carries the wrenches of row r % 64
        f = dev(torch, f_host)[torch.arange(B, device="cuda") % 64].contiguous()
    nv = desc.nv
    if layout == AOS:
        tau, tau_guard = poisoned(torch, B, (nv,), torch.float64)
        grad, grad_guard = poisoned(torch, B, (nv, nv), torch.float64)
        hm.gravity_gradient(q, GRAVITY, f, AOS, out=(tau, grad))
        tau_rows, grad_rows = tau, grad
    else:
        tau_t, tau_guard = poisoned(torch, nv, (B,), torch.float64)
        grad_t, grad_guard = poisoned(torch, nv * nv, (B,), torch.float64)
        hm.gravity_gradient(soa(torch, q), GRAVITY, soa(torch, f), SOA, out=(tau_t, grad_t))
        tau_rows, grad_rows = tau_t.t(), grad_t.t()
    torch.cuda.synchronize()
    q_idx = rows.rows(idx)[0]
    tau_ref, grad_ref = gc.gravity_gradient(desc, q_idx, GRAVITY, None if f_host is None else f_host[idx % 64])
    check_cover(tau_rows, tau_guard, idx, tau_ref, TOL, label="tau")
    check_cover(grad_rows, grad_guard, idx, grad_ref.reshape(len(idx), -1), TOL, label="grad")


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
    sys_, desc = make_case(case)
    _cover_case(torch_cuda, sys_, desc, B, None, layout, with_f=(B % 2 == 1))


def test_either_output_may_be_null_not_both(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 100
    q = dev(torch, states(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(25), B, desc.n_joints))
    tau, grad = hm.gravity_gradient(q, GRAVITY, f)
    tau_only, guard_t = poisoned(torch, B, (desc.nv,), torch.float64)
    grad_only, guard_g = poisoned(torch, B, (desc.nv, desc.nv), torch.float64)
    assert hm.gravity_gradient(q, GRAVITY, f, out=(tau_only, None))[1] is None
    assert hm.gravity_gradient(q, GRAVITY, f, out=(None, grad_only))[0] is None
    torch.cuda.synchronize()
    assert torch.equal(tau_only, tau) and torch.equal(grad_only, grad)
    assert torch.isnan(guard_t).all() and torch.isnan(guard_g).all()
    lib = _lib.load()
    g3 = (ctypes.c_double * 3)(*GRAVITY)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    assert lib.mh_gravity_gradient_f64(hm._h, B, q.data_ptr(), g3, None, ctypes.byref(opts), None, None) == 1  # MH_ERR_INVALID_ARGUMENT
    assert lib.mh_gravity_gradient_f32(hm._h, B, q.data_ptr(), g3, None, ctypes.byref(opts), None, None) == 1
    with pytest.raises(_lib.MecanoHipError):
        hm.gravity_gradient(q, GRAVITY, f, out=(None, None))


def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() the call is captured into a graph (it
    allocates nothing and clears nothing) and the replay gives the bits of the direct call, also on new inputs."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 1000
    q = dev(torch, states(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    tau_ref, grad_ref = hm.gravity_gradient(q, GRAVITY, f)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    tau, grad = torch.empty_like(tau_ref), torch.empty_like(grad_ref)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view.gravity_gradient(q, GRAVITY, f, out=(tau, grad))
        view.check(s.cuda_stream)
        assert torch.equal(tau, tau_ref) and torch.equal(grad, grad_ref)
        tau.zero_(), grad.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            view.gravity_gradient(q, GRAVITY, f, out=(tau, grad))
    torch.cuda.synchronize()
    assert not tau.any() and not grad.any()  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(tau, tau_ref) and torch.equal(grad, grad_ref)
    q2 = dev(torch, states(sys_, B, seed=6))
    tau_ref2, grad_ref2 = hm.gravity_gradient(q2, GRAVITY, f)
    q.copy_(q2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(tau, tau_ref2) and torch.equal(grad, grad_ref2)
    view.close()


def test_wrong_shapes_are_rejected_before_any_launch(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = HipModel(desc), 10, desc.nv, desc.n_joints
    q = dev(torch, states(sys_, B))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(B, n, 5), z(n * 6, B)):
        with pytest.raises(_lib.MecanoHipError):
            hm.gravity_gradient(q, GRAVITY, bad_f)
    with pytest.raises(_lib.MecanoHipError):
        hm.gravity_gradient(soa(torch, q), GRAVITY, z(B, n, 6), SOA)
    for bad_out in ((z(B, nv + 1), z(B, nv, nv)), (z(B, nv), z(B, nv, nv - 1)), (z(B - 1, nv), None), (None, z(nv * nv, B))):
        with pytest.raises(_lib.MecanoHipError):
            hm.gravity_gradient(q, GRAVITY, None, out=bad_out)
    check_bad_outputs(torch, [(B, nv), (B, nv, nv)], lambda out: hm.gravity_gradient(q, GRAVITY, None, out=out))
    with pytest.raises(_lib.MecanoHipError):
        hm.gravity_gradient(z(B, desc.nq + 1), GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.gravity_gradient(q, (0.0, 0.0, 0.0, 0.0, 0.0, -9.81))
    with pytest.raises(ValueError):
        hm.gravity_gradient(q, GRAVITY, torch.zeros((B, n, 6), dtype=torch.float32, device="cuda"))


def test_calculator_mirror(torch_cuda):
    """MultiBodyGravityGradientCalculator with the reference's names: the batched compute(q), and the one-configuration face that reads
    the joints' configuration; ignored subtrees are lumped."""
    from mecano_amd.calculators import MultiBodyGravityGradientCalculator
    from mecano_amd.multibody import JointStateType, MultiBodySystemTools
    torch = torch_cuda
    sys_, desc = make_case("lumped")
    calc = MultiBodyGravityGradientCalculator(sys_)
    assert calc.getInput() is sys_
    calc.setGravitionalAcceleration(GRAVITY)
    B = 50
    q = states(sys_, B)
    f = random_wrenches(np.random.default_rng(27), B, desc.n_joints, always=True)
    calc.setExternalWrenches(dev(torch, f))
    tau, grad = calc.compute(dev(torch, q))
    tau_ref, grad_ref = gc.gravity_gradient(desc, q, GRAVITY, f)  # desc: the lumped model
    close(tau.cpu().numpy(), tau_ref, TOL)
    close(grad.cpu().numpy(), grad_ref, TOL)
    assert calc.getTauMatrix() is tau and calc.getTauGradientMatrix() is grad
    # one configuration, the reference's way
    calc.setExternalWrenchesToZero()
    calc.setGravitionalAcceleration(-9.81)
    joints = sys_.getJointMatrixIndexProvider().getIndexedJointsInOrder()
    MultiBodySystemTools.insertJointsState(joints, JointStateType.CONFIGURATION, q[0].reshape(-1, 1))
    body = joints[-1].getSuccessor()
    wrench = np.array([1.0, -2.0, 3.0, -4.0, 5.0, -6.0])
    calc.setExternalWrench(body, wrench)
    assert np.array_equal(calc.getExternalWrench(body), wrench)
    f1 = np.zeros((1, desc.n_joints, 6))
    f1[0, -1] = wrench
    t1, g1 = gc.gravity_gradient(desc, q[:1], (0.0, 0.0, -9.81), f1)
    assert calc.getTauMatrix().shape == (desc.nv, 1) and calc.getTauGradientMatrix().shape == (desc.nv, desc.nv)
    close(calc.getTauMatrix().reshape(-1), t1[0], TOL)
    close(calc.getTauGradientMatrix(), g1[0], TOL)
    calc.setGravitionalAcceleration(0.0, 0.0, -1.0)
    calc.reset()
    t2, _ = gc.gravity_gradient(desc, q[:1], (0.0, 0.0, -1.0), f1)
    close(calc.getTauMatrix().reshape(-1), t2[0], TOL)


# ------------------------------------------------------------------------------------------------ scattered index maps
@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    """Configurations and wrenches in the identity description's index space and the checker's outputs on them: once per model and
    precision, shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if dtype_name == "float32" else np.float64
    q = DistinctRows(sys_, 16, seed=43).rows(np.arange(70), np_dt)[0]
    f = random_wrenches(np.random.default_rng(44), 70, d0.n_joints).astype(np_dt).astype(np.float64)
    return q, f, gc.gravity_gradient(d0, q, GRAVITY, f)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """The device on a description whose maps send every DoF and every configuration entry somewhere else (with holes: two indices of
    each space owned by no joint), on moved configurations, against the checker on the IDENTITY description: tau and the gradient moved
    back meet this file's bounds (1e-10, f32_forward_tol(2 n) in fp32), the guard rows stay poisoned, and with the rows or the columns left
    where they are the gradient misses the reference by more than 1e-3."""
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv = hp.scattered_model(d, model), 70, d.nv
    q, f, (tau_ref, grad_ref) = _scattered_reference(model, dtype_name)
    tol = TOL if dtype_name == "float64" else f32_forward_tol(2 * d0.n_joints)
    is_soa = layout == SOA
    outs, guards = hp.poisoned_set(torch, B, [(nv,), (nv, nv)], dtype, is_soa)
    tq, tf = dev(torch, hp.to_q(q, pq, d.nq), dtype), dev(torch, f, dtype)
    if is_soa:
        tq, tf = soa(torch, tq), soa(torch, tf)
    hm.gravity_gradient(tq, GRAVITY, tf, layout, out=tuple(outs))
    torch.cuda.synchronize()
    hp.guards_intact(guards, "gravity_gradient")
    tau, grad = hp.rows_of(outs[0], B, (nv,), is_soa), hp.rows_of(outs[1], B, (nv, nv), is_soa)
    close(hp.from_v(tau, pv)[0], tau_ref, tol, label="scattered tau")
    close(hp.from_vv(grad, pv)[0], grad_ref, tol, label="scattered grad")
    hp.assert_misses(hp.keep_order(tau, pv), tau_ref, "tau")
    hp.assert_misses(hp.keep_order(grad, pv, (-2,))[:, :, pv], grad_ref, "grad, rows left where they are")
    hp.assert_misses(hp.keep_order(grad, pv, (-1,))[:, pv, :], grad_ref, "grad, columns left where they are")
