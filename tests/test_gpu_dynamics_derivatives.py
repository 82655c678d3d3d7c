"""mh_rnea_derivatives_* / mh_aba_derivatives_* on the device against the CPU checker (tests/dynamics_derivatives_check.py, pinned by
tests/test_dynamics_derivatives_cpu.py) and against the device's own neighbours (rnea, aba, gravity_gradient, mass_matrix_inverse),
through the C-ABI (the HipModel methods are the ctypes calls)."""
import functools

import numpy as np
import pytest

import dynamics_derivatives_check as dc
import gravity_gradient_check as gc
import helpers as hp
from helpers import DistinctRows, check_bad_outputs, check_cover, close, close_aba, f32_forward_tol, group_cover, poisoned
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches, system_of

pytestmark = pytest.mark.gpu

TOL = 1.0e-10  # helpers.close default: relative to max(1, |ref|_inf)
AOS, SOA = 0, 1
U32 = 2.0 ** -24
ROOT_ACC = np.array([0.4, -0.3, 0.2, 1.5, -0.7, 9.0])
TREE_ROWS = np.array([0, 1, 31, 63, 64, 69])  # (the checker takes seconds per row of the 128-body tree)


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


def state(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)


def tree128():
    sys_ = system_of(rt.nextJointTree(np.random.default_rng(17), 128, ("revolute", "prismatic", "sixdof")))
    return sys_, sys_.toModelDesc()


def to_host(torch, outs, B, nv, layout):
    """Device outputs -> AoS-shaped fp64 numpy ([B, nv] vectors, [B, nv, nv] matrices); None stays None."""
    torch.cuda.synchronize()
    res = []
    for t in outs:
        if t is None:
            res.append(None)
            continue
        a = (t.t() if layout == SOA else t).cpu().numpy().astype(np.float64)
        res.append(a.reshape(B, nv) if a.size == B * nv else a.reshape(B, nv, nv))
    return tuple(res)


def run_rnea(torch, hm, q, qd, qdd, f, layout, gravity=GRAVITY, dtype=None, **kw):
    args = [dev(torch, x, dtype) for x in (q, qd, qdd, f)]
    if layout == SOA:
        args = [soa(torch, x) for x in args]
    return to_host(torch, hm.rnea_derivatives(args[0], args[1], args[2], gravity, args[3], layout, **kw), q.shape[0], hm.nv, layout)


def run_aba(torch, hm, q, qd, tau, f, layout, gravity=GRAVITY, dtype=None, **kw):
    args = [dev(torch, x, dtype) for x in (q, qd, tau, f)]
    if layout == SOA:
        args = [soa(torch, x) for x in args]
    return to_host(torch, hm.aba_derivatives(args[0], args[1], args[2], gravity, args[3], layout, **kw), q.shape[0], hm.nv, layout)


# ------------------------------------------------------------------------------------------------ inverse dynamics
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("wrenches", ["none", "zero", "random"])
def test_fp64_matches_checker(torch_cuda, case, layout, wrenches):
    """Every model of the CPU pins, both layouts, without f_ext, with an all-zero f_ext and with random wrenches; 70 states: one full
    group of 64 and a ragged one, split over several waves per group (the parts of small batches)."""
    from mecano_amd.engine import HipModel
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 70
    q, qd, qdd, _ = state(sys_, B)
    f = {"none": None, "zero": np.zeros((B, desc.n_joints, 6)),
         "random": random_wrenches(np.random.default_rng(21), B, desc.n_joints)}[wrenches]
    tau, dq, dqd = run_rnea(torch_cuda, hm, q, qd, qdd, f, layout)
    tau_ref, dq_ref, dqd_ref = dc.rnea_derivatives(desc, q, qd, qdd, GRAVITY, f)
    close(tau, tau_ref, TOL, label="tau")
    close(dq, dq_ref, TOL, label="dtau_dq")
    close(dqd, dqd_ref, TOL, label="dtau_dqd")
    unrelated = ~gc.related(desc)
    assert np.all(dq[:, unrelated] == 0.0) and np.all(dqd[:, unrelated] == 0.0)  # written, and exactly zero


@pytest.mark.parametrize("case", ["arm7", "humanoid30", "tree128"])
def test_fp32_matches_checker(torch_cuda, case):
    """fp32 on the arm, the humanoid and the 128-body random tree of the gravity test.  Bound, fixed before any run: the gravity test's
    argument (an inward accumulation over a subtree of up to n bodies followed by a climb over up to n ancestors) with the outward
    velocity / acceleration sweep as a third pass -- a recursion over at most 3 n bodies in helpers.f32_forward_tol's terms, relative to
    max(1, |ref|_inf).  The checker runs in fp64 on the fp32-rounded inputs.  On the tree the rows TREE_ROWS are compared; every row
    must be free of NaN."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = tree128() if case == "tree128" else make_case(case)
    hm, B = HipModel(desc), 70
    q, qd, qdd, _ = (x.astype(np.float32) for x in state(sys_, B))
    f = random_wrenches(np.random.default_rng(22), B, desc.n_joints).astype(np.float32)
    tol = f32_forward_tol(3 * desc.n_joints)
    rows = np.arange(B) if case != "tree128" else TREE_ROWS
    m = dc.DerivativeModel(desc)
    ref = dc.rnea_derivatives(m, q.astype(np.float64), qd.astype(np.float64), qdd.astype(np.float64), GRAVITY, f.astype(np.float64), rows=rows)
    for layout in (AOS, SOA):
        got = run_rnea(torch, hm, q, qd, qdd, f, layout, dtype=torch.float32)
        for g, r, name in zip(got, ref, ("tau", "dtau_dq", "dtau_dqd")):
            assert not np.isnan(g).any()
            close(g[rows], r[rows], tol, label=f"fp32 {name} layout {layout}")


@pytest.mark.parametrize("case", CASES)
def test_consistent_with_the_device_neighbours(torch_cuda, case):
    """tau is the device's inverse dynamics; at rest the matrix is the device's gravity gradient; with a root acceleration set the
    velocity matrix obeys (d tau / d qd) qd = 2 (rnea(q, qd, qdd) - rnea(q, 0, qdd)), evaluated with two device calls."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B = HipModel(desc), 200
    q, qd, qdd, _ = (dev(torch, x) for x in state(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(23), B, desc.n_joints))
    z = torch.zeros_like(qd)
    for fe in (None, f):
        tau, dq, dqd = hm.rnea_derivatives(q, qd, qdd, GRAVITY, fe)
        close(tau.cpu().numpy(), hm.rnea(q, qd, qdd, GRAVITY, fe).cpu().numpy(), TOL, label="tau vs rnea")
        _, dq0, dqd0 = hm.rnea_derivatives(q, z, z, GRAVITY, fe)
        close(dq0.cpu().numpy(), hm.gravity_gradient(q, GRAVITY, fe)[1].cpu().numpy(), TOL, label="at rest vs gravity_gradient")
        assert not dqd0.any()
        tau, _, dqd = hm.rnea_derivatives(q, qd, qdd, ROOT_ACC, fe)
        t1, t0 = hm.rnea(q, qd, qdd, ROOT_ACC, fe), hm.rnea(q, z, qdd, ROOT_ACC, fe)
        close(tau.cpu().numpy(), t1.cpu().numpy(), TOL, label="tau vs rnea, root acceleration")
        close(torch.einsum("bij,bj->bi", dqd, qd).cpu().numpy(), (2.0 * (t1 - t0)).cpu().numpy(), TOL, label="homogeneity")


def test_switches(torch_cuda):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 100
    q, qd, qdd, _ = (dev(torch, x) for x in state(sys_, B))
    z = torch.zeros_like(qd)
    off = hm.rnea_derivatives(q, None, qdd, GRAVITY, consider_coriolis=False)
    ref = hm.rnea_derivatives(q, z, qdd, GRAVITY)
    assert all(torch.equal(a, b) for a, b in zip(off, ref)) and not off[2].any()
    off = hm.rnea_derivatives(q, qd, None, GRAVITY, consider_accelerations=False)
    ref = hm.rnea_derivatives(q, qd, z, GRAVITY)
    assert all(torch.equal(a, b) for a, b in zip(off, ref))


# ------------------------------------------------------------------------------------------------ forward dynamics
def _forward_case(torch, sys_, desc, B, layout, dtype, u, rows=None, with_f=True):
    """Device forward-dynamics derivatives against the device's aba and mass_matrix_inverse and against the checker, the matrices with
    the per-configuration bound of helpers.close_aba's form: 8 sqrt(8 * 3 n) cond_inf(H) u max(1, |ref|_inf), cond from the oracle's H."""
    from mecano_amd.engine import HipModel
    hm = HipModel(desc)
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    q, qd, _, tau = (x.astype(np_dt) for x in state(sys_, B))
    f = random_wrenches(np.random.default_rng(31), B, desc.n_joints).astype(np_dt) if with_f else None
    qdd, Dq, Dv, Hinv = run_aba(torch, hm, q, qd, tau, f, layout, dtype=dtype)
    for x in (qdd, Dq, Dv, Hinv):
        assert not np.isnan(x).any()
    dq_, dqd_, dtau_, df_ = dev(torch, q, dtype), dev(torch, qd, dtype), dev(torch, tau, dtype), dev(torch, f, dtype)
    qdd_dev = hm.aba(dq_, dqd_, dtau_, GRAVITY, df_).cpu().numpy().astype(np.float64)
    Hinv_dev = hm.mass_matrix_inverse(dq_).cpu().numpy().astype(np.float64)
    assert np.array_equal(Hinv, Hinv_dev)  # the same launch on the same inputs
    if not np.array_equal(qdd, qdd_dev):  # (forward dynamics may take another plan beside other launches)
        close_aba(qdd, qdd_dev, OracleModel(desc).crba(q.astype(np.float64)), desc.n_joints, u, label="qdd vs aba")
    rows = np.arange(B) if rows is None else rows
    q64, qd64, tau64 = q.astype(np.float64), qd.astype(np.float64), tau.astype(np.float64)
    f64 = None if f is None else f.astype(np.float64)
    _, Dq_ref, Dv_ref, _ = dc.aba_derivatives(desc, q64, qd64, tau64, GRAVITY, f64, rows=rows)
    H = OracleModel(desc).crba(q64[rows])
    n3 = 3 * desc.n_joints
    close_aba(Dq[rows].reshape(len(rows), -1), Dq_ref[rows].reshape(len(rows), -1), H, n3, u, label=f"dqdd_dq layout {layout}")
    close_aba(Dv[rows].reshape(len(rows), -1), Dv_ref[rows].reshape(len(rows), -1), H, n3, u, label=f"dqdd_dqd layout {layout}")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_fp64_matches_checker(torch_cuda, case, layout):
    sys_, desc = make_case(case)
    _forward_case(torch_cuda, sys_, desc, 70, layout, torch_cuda.float64, 2.0 ** -53, with_f=(layout == AOS))


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_forward_fp32_matches_checker(torch_cuda, case):
    sys_, desc = make_case(case)
    for layout in (AOS, SOA):
        _forward_case(torch_cuda, sys_, desc, 70, layout, torch_cuda.float32, 2.0 ** -24)


def test_forward_on_the_tree_beyond_what_lds_holds(torch_cuda):
    """The committed 128-body benchmark tree, nv = 323: a 323 x 323 matrix does not fit LDS; the product kernel goes through it in
    chunks of columns."""
    sys_ = rt.committedBenchmarkSystems()["tree128"]
    desc = sys_.toModelDesc()
    assert desc.nv == 323
    _forward_case(torch_cuda, sys_, desc, 70, AOS, torch_cuda.float64, 2.0 ** -53, rows=TREE_ROWS)


# ------------------------------------------------------------------------------------------------ cover of batches
def _cover_case(torch, sys_, desc, B, grid, layout, with_f, skip=None, forward=False):
    """B distinct rows, poisoned outputs with a guard row behind them, every row group checked against the checker; `skip`: index of
    the output passed as NULL."""
    from mecano_amd.engine import HipModel
    hm = HipModel(desc)
    rows = DistinctRows(sys_, 256, seed=29)
    q, qd, qdd, tau = rows.device(torch, B)
    idx = group_cover(B, grid)
    f_host = random_wrenches(np.random.default_rng(24), 64, desc.n_joints) if with_f else None
    f = dev(torch, f_host)[torch.arange(B, device="cuda") % 64].contiguous() if with_f else None
    nv = desc.nv
    shapes = [(nv,), (nv, nv), (nv, nv)] + ([(nv, nv)] if forward else [])
    outs, guards = [], []
    for k, s in enumerate(shapes):
        if k == skip:
            outs.append(None), guards.append(None)
            continue
        o, g = poisoned(torch, B, s, torch.float64) if layout == AOS else poisoned(torch, int(np.prod(s)), (B,), torch.float64)
        outs.append(o), guards.append(g)
    x3 = tau if forward else qdd
    args = (q, qd, x3, GRAVITY, f) if layout == AOS else (soa(torch, q), soa(torch, qd), soa(torch, x3), GRAVITY, soa(torch, f))
    (hm.aba_derivatives if forward else hm.rnea_derivatives)(*args, layout, out=tuple(outs))
    torch.cuda.synchronize()
    qi, qdi, qddi, taui = rows.rows(idx)
    fi = None if f_host is None else f_host[idx % 64]
    if forward:
        ref = dc.aba_derivatives(desc, qi, qdi, taui, GRAVITY, fi)
        conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(qi)])
    else:
        ref = dc.rnea_derivatives(desc, qi, qdi, qddi, GRAVITY, fi)
    for k, (o, g, r) in enumerate(zip(outs, guards, ref)):
        if o is None:
            continue
        o_rows = o if layout == AOS else o.t()
        if forward:  # guard intact, no row left unwritten; the values with the conditioned bound of the forward-dynamics tests
            assert torch.isnan(g).all(), f"output {k}: wrote past the last row"
            assert not torch.isnan(o).any(), f"output {k}: rows left unwritten (NaN)"
            close_aba(_rows_of(o_rows, idx).reshape(len(idx), -1), r.reshape(len(idx), -1), None, 3 * desc.n_joints, conds=conds,
                      label=f"output {k}")
        else:
            check_cover(o_rows, g, idx, r.reshape(len(idx), -1), TOL, label=f"output {k}")


def _rows_of(t, idx):
    import torch
    return t[torch.as_tensor(np.asarray(idx), device=t.device)].cpu().numpy().astype(np.float64)


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


@pytest.mark.parametrize("skip", [0, 1, 2])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_each_output_null_in_turn(torch_cuda, skip, layout):
    sys_, desc = make_case("humanoid30")
    _cover_case(torch_cuda, sys_, desc, 64 * 5 + 3, None, layout, with_f=True, skip=skip)


@pytest.mark.parametrize("skip", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_forward_covers_every_row_group_each_output_null_in_turn(torch_cuda, skip, layout):
    sys_, desc = make_case("humanoid30")
    _cover_case(torch_cuda, sys_, desc, 64 * 5 + 3, None, layout, with_f=True, skip=skip, forward=True)


# ------------------------------------------------------------------------------------------------ plumbing
def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() both calls are captured into a graph
    (they allocate nothing) and the replay gives the bits of the direct call, also on new inputs."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = HipModel(desc), 1000
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    ref_i = hm.rnea_derivatives(q, qd, qdd, GRAVITY, f)
    ref_f = hm.aba_derivatives(q, qd, tau, GRAVITY, f)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    out_i = tuple(torch.empty_like(t) for t in ref_i)
    out_f = tuple(torch.empty_like(t) for t in ref_f[1:3])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view.rnea_derivatives(q, qd, qdd, GRAVITY, f, out=out_i)
        view.aba_derivatives(q, qd, tau, GRAVITY, f, out=(None, out_f[0], out_f[1], None))  # qdd and Hinv in the context's scratch
        view.check(s.cuda_stream)
        assert all(torch.equal(a, b) for a, b in zip(out_i, ref_i)) and all(torch.equal(a, b) for a, b in zip(out_f, ref_f[1:3]))
        for t in out_i + out_f:
            t.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            view.rnea_derivatives(q, qd, qdd, GRAVITY, f, out=out_i)
            view.aba_derivatives(q, qd, tau, GRAVITY, f, out=(None, out_f[0], out_f[1], None))
    torch.cuda.synchronize()
    assert not any(t.any() for t in out_i + out_f)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out_i, ref_i)) and all(torch.equal(a, b) for a, b in zip(out_f, ref_f[1:3]))
    q2 = dev(torch, state(sys_, B, seed=6)[0])
    ref_i2 = hm.rnea_derivatives(q2, qd, qdd, GRAVITY, f)
    ref_f2 = hm.aba_derivatives(q2, qd, tau, GRAVITY, f)
    q.copy_(q2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out_i, ref_i2)) and all(torch.equal(a, b) for a, b in zip(out_f, ref_f2[1:3]))
    view.close()


def test_wrong_shapes_are_rejected_before_any_launch(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = HipModel(desc), 10, desc.nv, desc.n_joints
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6), z(B, n, 5), z(n * 6, B)):
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_derivatives(q, qd, qdd, GRAVITY, bad_f)
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_derivatives(q, qd, tau, GRAVITY, bad_f)
    for bad_out in ((z(B, nv + 1), z(B, nv, nv), None), (None, z(B, nv, nv - 1), None), (None, None, z(nv * nv, B)), (None, None, None),
                    (None, z(B, nv, nv))):
        with pytest.raises(_lib.MecanoHipError):
            hm.rnea_derivatives(q, qd, qdd, GRAVITY, None, out=bad_out)
    for bad_out in ((None, None, None, z(B, nv, nv)), (z(B, nv), z(B, nv, nv + 1), None, None), (None, z(B, nv, nv), None, z(B, nv))):
        with pytest.raises(_lib.MecanoHipError):
            hm.aba_derivatives(q, qd, tau, GRAVITY, None, out=bad_out)
    vec, mat = (B, nv), (B, nv, nv)
    check_bad_outputs(torch, [vec, mat, mat], lambda out: hm.rnea_derivatives(q, qd, qdd, GRAVITY, None, out=out))
    check_bad_outputs(torch, [vec, mat, mat, mat], lambda out: hm.aba_derivatives(q, qd, tau, GRAVITY, None, out=out))
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_derivatives(q, z(B, nv + 1), qdd, GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_derivatives(q, qd, None, GRAVITY)
    with pytest.raises(_lib.MecanoHipError):
        hm.rnea_derivatives(q, qd, qdd, (0.0, -9.81))
    with pytest.raises(ValueError):
        hm.rnea_derivatives(q, qd, qdd, GRAVITY, torch.zeros((B, n, 6), dtype=torch.float32, device="cuda"))


def test_calculator_mirrors(torch_cuda):
    from mecano_amd.calculators import ForwardDynamicsCalculator, InverseDynamicsCalculator
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    B = 40
    q, qd, qdd, tau = state(sys_, B)
    f = random_wrenches(np.random.default_rng(27), B, desc.n_joints, always=True)
    inv = InverseDynamicsCalculator(sys_)
    inv.setGravitationalAcceleration(*GRAVITY)
    inv.setExternalWrenches(dev(torch, f))
    got = inv.getJointTauGradients(dev(torch, q), dev(torch, qd), dev(torch, qdd))
    for g, r in zip(got, dc.rnea_derivatives(desc, q, qd, qdd, GRAVITY, f)):
        close(g.cpu().numpy(), r, TOL)
    inv.setConsiderCoriolisAndCentrifugalForces(False)
    got = inv.getJointTauGradients(dev(torch, q), dev(torch, qd), dev(torch, qdd))
    for g, r in zip(got, dc.rnea_derivatives(desc, q, qd, qdd, GRAVITY, f, consider_coriolis=False)):
        close(g.cpu().numpy(), r, TOL)
    fwd = ForwardDynamicsCalculator(sys_)
    fwd.setGravitationalAcceleration(*GRAVITY)
    fwd.setExternalWrenches(dev(torch, f))
    qdd_d, Dq, Dv, Hinv = fwd.getJointAccelerationGradients(dev(torch, q), dev(torch, qd), dev(torch, tau))
    ref = dc.aba_derivatives(desc, q, qd, tau, GRAVITY, f)
    H = OracleModel(desc).crba(q)
    for g, r in zip((qdd_d, Dq, Dv, Hinv), ref):
        close_aba(g.cpu().numpy().reshape(B, -1), r.reshape(B, -1), H, 3 * desc.n_joints)


# ------------------------------------------------------------------------------------------------ scattered index maps
@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    """Inputs in the identity description's index space and the checker's outputs on them: computed once per model and precision (the
    states rounded to it), shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if dtype_name == "float32" else np.float64
    q, qd, qdd, tau = DistinctRows(sys_, 16, seed=41).rows(np.arange(70), np_dt)
    f = random_wrenches(np.random.default_rng(42), 70, d0.n_joints).astype(np_dt).astype(np.float64)
    inv = dc.rnea_derivatives(d0, q, qd, qdd, GRAVITY, f)
    fwd = dc.aba_derivatives(d0, q, qd, tau, GRAVITY, f)
    conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(d0).crba(q)])
    assert conds.max() < 1.0e8
    return (q, qd, qdd, tau, f), inv, fwd, conds


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """rnea_derivatives and aba_derivatives on a description whose maps send every DoF and every configuration entry somewhere else (the
    parts of a quaternion apart; with holes, two indices of each space owned by no joint), on moved inputs, against the checker on the
    IDENTITY description: every output moved back meets this file's own bounds (1e-10 resp. f32_forward_tol(3 n) for the inverse form,
    close_aba's per-row cond_inf(H) bound for the forward form), the guard rows stay poisoned, and read without moving rows or columns
    back the same outputs miss the reference by more than 1e-3."""
    torch = torch_cuda
    dtype, u = getattr(torch, dtype_name), (U32 if dtype_name == "float32" else 2.0 ** -53)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, n = hp.scattered_model(d, model), 70, d.nv, d0.n_joints
    (q, qd, qdd, tau, f), inv, fwd, conds = _scattered_reference(model, dtype_name)
    is_soa = layout == SOA
    lay = (lambda x: soa(torch, x)) if is_soa else (lambda x: x)
    tq, tqd, tqdd, ttau = (lay(dev(torch, x, dtype)) for x in (hp.to_q(q, pq, d.nq), hp.to_v(qd, pv, nv), hp.to_v(qdd, pv, nv), hp.to_v(tau, pv, nv)))
    tf = lay(dev(torch, f, dtype))
    tol = TOL if dtype_name == "float64" else f32_forward_tol(3 * n)
    # the inverse form
    outs, guards = hp.poisoned_set(torch, B, [(nv,), (nv, nv), (nv, nv)], dtype, is_soa)
    hm.rnea_derivatives(tq, tqd, tqdd, GRAVITY, tf, layout, out=tuple(outs))
    torch.cuda.synchronize()
    hp.guards_intact(guards, "rnea_derivatives")
    got = [hp.rows_of(o, B, s, is_soa) for o, s in zip(outs, [(nv,), (nv, nv), (nv, nv)])]
    close(hp.from_v(got[0], pv)[0], inv[0], tol, label="scattered tau")
    hp.assert_misses(hp.keep_order(got[0], pv), inv[0], "tau")
    for k, name in ((1, "dtau_dq"), (2, "dtau_dqd")):
        close(hp.from_vv(got[k], pv)[0], inv[k], tol, label=f"scattered {name}")
        hp.assert_misses(hp.keep_order(got[k], pv, (-2,))[:, :, pv], inv[k], f"{name}, rows left where they are")
        hp.assert_misses(hp.keep_order(got[k], pv, (-1,))[:, pv, :], inv[k], f"{name}, columns left where they are")
    # the forward form
    shapes = [(nv,), (nv, nv), (nv, nv), (nv, nv)]
    outs, guards = hp.poisoned_set(torch, B, shapes, dtype, is_soa)
    hm.aba_derivatives(tq, tqd, ttau, GRAVITY, tf, layout, out=tuple(outs))
    torch.cuda.synchronize()
    hp.guards_intact(guards, "aba_derivatives")
    got = [hp.rows_of(o, B, s, is_soa) for o, s in zip(outs, shapes)]
    close_aba(hp.from_v(got[0], pv)[0], fwd[0], None, n, u, label="scattered qdd", conds=conds)
    hp.assert_misses(hp.keep_order(got[0], pv), fwd[0], "qdd")
    for k, name, bodies in ((1, "dqdd_dq", 3 * n), (2, "dqdd_dqd", 3 * n), (3, "Hinv", 3 * n)):
        close_aba(hp.from_vv(got[k], pv)[0].reshape(B, -1), fwd[k].reshape(B, -1), None, bodies, u, label=f"scattered {name}", conds=conds)
        hp.assert_misses(hp.keep_order(got[k], pv, (-2,))[:, :, pv], fwd[k], f"{name}, rows left where they are")
        hp.assert_misses(hp.keep_order(got[k], pv, (-1,))[:, pv, :], fwd[k], f"{name}, columns left where they are")
