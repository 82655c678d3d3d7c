"""mh_apparent_inertia_inverse_f64 / _f32 on the device against the CPU checker (tests/apparent_inertia_check.py, pinned by
tests/test_apparent_inertia_cpu.py), through the C-ABI (HipModel.apparent_inertia_inverse is the ctypes call) and the calculator mirror."""
import ctypes
import functools

import numpy as np
import pytest

import apparent_inertia_check as ac
import helpers as hp
from helpers import DistinctRows, check_bad_outputs, check_cover, f32_aba_forward_factor, group_cover, poisoned, record_parity
from test_apparent_inertia_cpu import CASES, HUMANOID_TARGETS, WELL_CONDITIONED, make_case, states, targets_of

pytestmark = pytest.mark.gpu

AOS, SOA = 0, 1
DIAGONAL, COUPLED = 0, 1
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def model_of(desc, locked):
    from mecano_amd.engine import HipModel
    hm = HipModel(desc)
    if locked is not None:
        hm.set_joint_source_modes(locked)
    return hm


def run(torch, hm, q, targets, poses, coupled, layout, dtype=None):
    """Device call on a host array laid out as the call wants it; returns AoS-shaped fp64 numpy."""
    dq = dev(torch, q, dtype)
    if layout == SOA:
        dq = dq.t().contiguous()
    W = hm.apparent_inertia_inverse(dq, targets, poses, coupled, layout)
    torch.cuda.synchronize()
    B, K = q.shape[0], len(targets)
    if layout == SOA:
        W = W.t()
    return W.cpu().numpy().astype(np.float64).reshape((B, 6 * K, 6 * K) if coupled else (B, K, 6, 6))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_fp64_matches_checker(torch_cuda, case, layout):
    """Every family, both layouts, both block modes, without poses and with random ones, 1 / 3 / 16 targets (from 3 on one body is named
    twice); 70 configurations: one full group of 64 and a ragged one, the sources split over several waves per group."""
    from oracle.cpu_oracle import OracleModel
    sys_, desc, locked = make_case(case)
    hm, om, B = model_of(desc, locked), OracleModel(desc), 70
    q = states(sys_, B)
    bounds = ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED)
    for K in (1, 3, 16):
        t = targets_of(case, desc, K)
        for poses in (None, ac.random_poses(np.random.default_rng(31 + K), K)):
            for coupled in (False, True):
                W = run(torch_cuda, hm, q, t, poses, coupled, layout)
                ref = ac.apparent_inertia_inverse(om, q, t, poses, coupled, locked)
                ac.close_rows(W, ref, bounds, label=f"{case} K={K} {'coupled' if coupled else 'diagonal'} poses={poses is not None}")


@pytest.mark.parametrize("case", ["arm7", "humanoid30", "tree128"])
def test_fp32_matches_fp64_checker(torch_cuda, case):
    """fp32 against the fp64 checker on the fp32-rounded configurations.  The bound is helpers.close_aba's form with u = 2^-24: W's
    columns are forward-dynamics solves, so |W - ref|_inf <= 8 sqrt(8 n) cond_inf(H) u max(1, |ref|_inf) per configuration
    (f32_aba_forward_factor); achieved / bound is recorded."""
    from oracle.cpu_oracle import OracleModel
    torch = torch_cuda
    sys_, desc, _ = make_case(case)
    hm, om, B = model_of(desc, None), OracleModel(desc), 70
    q = states(sys_, B).astype(np.float32)
    q64 = q.astype(np.float64)
    t = targets_of(case, desc, 4)
    poses = ac.random_poses(np.random.default_rng(33), 4)
    conds = ac.mass_matrix_conds(om, q64)
    factor = f32_aba_forward_factor(desc.n_joints)
    ref = ac.apparent_inertia_inverse(om, q64, t, poses, True)
    scale = np.maximum(1.0, np.abs(ref).reshape(B, -1).max(axis=1))
    for layout in (AOS, SOA):
        W = run(torch, hm, q, t, poses, True, layout, torch.float32)
        assert not np.isnan(W).any()
        rel = np.abs(W - ref).reshape(B, -1).max(axis=1) / scale
        ratio = float((rel / (conds * 2.0 ** -24)).max())
        print(f"{case} fp32 layout {layout}: err / (cond u) = {ratio:.3e}, factor {factor:.3e}, achieved / bound = {ratio / factor:.3e}")
        record_parity(ratio, factor, f"fp32 {case} layout {layout} err / (cond_inf(H) u)")
        assert ratio <= factor


@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    """Configurations in the identity description's index space and the checker's W in both block modes: once per model and precision,
    shared by the layouts, the hole and the re-listing cases, never modified."""
    from oracle.cpu_oracle import OracleModel
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    om, B = OracleModel(d0), 70
    q = DistinctRows(sys_, 16, seed=81).rows(np.arange(B), np.float32 if dtype_name == "float32" else np.float64)[0]
    t = list(HUMANOID_TARGETS) + [HUMANOID_TARGETS[1]] if model == "humanoid30" else [d0.n_joints - 1, 4, 2, 4]  # one body named twice
    poses = ac.random_poses(np.random.default_rng(82), len(t))
    refs = {coupled: ac.apparent_inertia_inverse(om, q, t, poses, coupled) for coupled in (False, True)}
    conds = ac.mass_matrix_conds(om, q)
    assert conds.max() < 1.0e8
    return q, t, poses, refs, ac.bound_of(om, q, d0.n_joints, False), conds


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes,relist", [("mixed10", 0, False), ("mixed10", 2, False), ("humanoid30", 0, False), ("humanoid30", 0, True)])
def test_scattered_index_maps(torch_cuda, model, holes, relist, layout, dtype_name):
    """Both block modes on a description whose configuration map sends every entry somewhere else (with holes: two indices owned by no
    joint, holding 7.0 in q), against the checker on the IDENTITY description: only q moves, W does not.  fp64 under ac.bound_of's per-row
    bound, fp32 under test_fp32_matches_fp64_checker's f32_aba_forward_factor(n) cond_inf(H) 2^-24 max(1, |ref|_inf).  relist: the
    scattered description's joints are listed in a random order, parents possibly after their children, and the target list is
    translated.  The guard row stays poisoned; fed q as the identity description lists it the call misses the reference by more than
    1e-3."""
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    q, t, poses, refs, bounds, conds = _scattered_reference(model, dtype_name)
    if relist:
        d, order = hp.relisted(d, np.random.default_rng(83))
        assert any(d.parent[k] > k for k in range(d.n_joints)) and hp.maps_flags(d) == (0, 1)
        t = [int(np.argsort(order)[j]) for j in t]
    hm, B, K = hp.scattered_model(d, model) if not relist else model_of(d, None), 70, len(t)
    is_soa = layout == SOA
    for coupled in (False, True):
        shape = (6 * K, 6 * K) if coupled else (K, 6, 6)
        (W,), guards = hp.poisoned_set(torch, B, [shape], dtype, is_soa)
        tq = dev(torch, hp.to_q(q, pq, d.nq), dtype)
        hm.apparent_inertia_inverse(tq.t().contiguous() if is_soa else tq, t, poses, coupled, layout, out=W)
        torch.cuda.synchronize()
        hp.guards_intact(guards, "apparent_inertia_inverse")
        got, ref = hp.rows_of(W, B, shape, is_soa), refs[coupled]
        assert not np.isnan(got).any()
        label = f"scattered {model} holes={holes} relist={relist} {'coupled' if coupled else 'diagonal'} layout {layout} {dtype_name}"
        if dtype_name == "float64":
            ac.close_rows(got, ref, bounds, label=label)
        else:
            rel = np.abs(got - ref).reshape(B, -1).max(axis=1) / np.maximum(1.0, np.abs(ref).reshape(B, -1).max(axis=1))
            ratio, factor = float((rel / (conds * 2.0 ** -24)).max()), f32_aba_forward_factor(d0.n_joints)
            record_parity(ratio, factor, label + " err / (cond_inf(H) u)")
            assert ratio <= factor, f"{label}: {ratio:.3e} > {factor:.3e}"
        if not holes:
            unmoved = hm.apparent_inertia_inverse(dev(torch, q, dtype).t().contiguous() if is_soa else dev(torch, q, dtype), t, poses, coupled, layout)
            torch.cuda.synchronize()
            hp.assert_misses(hp.rows_of(unmoved, B, shape, is_soa), ref, label + ", q unmoved")


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("coupled", [False, True])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout, coupled):
    """More than twice the waves the grid holds (8 per CU), plus a ragged last group: every lane loops over several groups of 64.  B
    distinct rows, a poisoned output with a guard row behind it, every row group checked, every entry written."""
    from oracle.cpu_oracle import OracleModel
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    sys_, desc, _ = make_case("humanoid30")
    hm, om = model_of(desc, None), OracleModel(desc)
    B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
    rows = DistinctRows(sys_, 256, seed=29)
    q = rows.device(torch, B)[0]
    idx = group_cover(B, grid)
    K = len(HUMANOID_TARGETS)
    size = 36 * K * K if coupled else 36 * K
    poses = ac.random_poses(np.random.default_rng(34), K)
    if layout == AOS:
        W, guard = poisoned(torch, B, (6 * K, 6 * K) if coupled else (K, 6, 6), torch.float64)
        hm.apparent_inertia_inverse(q, HUMANOID_TARGETS, poses, coupled, AOS, out=W)
        W_rows = W
    else:
        W_t, guard = poisoned(torch, size, (B,), torch.float64)
        hm.apparent_inertia_inverse(q.t().contiguous(), HUMANOID_TARGETS, poses, coupled, SOA, out=W_t)
        W_rows = W_t.t()
    torch.cuda.synchronize()
    ref = ac.apparent_inertia_inverse(om, rows.rows(idx)[0], HUMANOID_TARGETS, poses, coupled)
    check_cover(W_rows, guard, idx, ref.reshape(len(idx), -1), 1.0e-10, label="W")


def test_small_ragged_batches_and_guards(torch_cuda):
    from oracle.cpu_oracle import OracleModel
    torch = torch_cuda
    sys_, desc, _ = make_case("onedof_tree")
    hm, om = model_of(desc, None), OracleModel(desc)
    t = targets_of("onedof_tree", desc, 5)
    for B in (1, 63, 64 * 3 + 1, 4096):
        q = states(sys_, B)
        bounds = ac.bound_of(om, q, desc.n_joints, False)
        W, guard = poisoned(torch, B, (30, 30), torch.float64)
        hm.apparent_inertia_inverse(dev(torch, q), t, None, True, AOS, out=W)
        torch.cuda.synchronize()
        assert torch.isnan(guard).all() and not torch.isnan(W).any()
        ac.close_rows(W.cpu().numpy(), ac.apparent_inertia_inverse(om, q, t, None, True), bounds, label=f"B={B}")


def test_locked_joints_and_back(torch_cuda):
    """Two acceleration-source joints: the device matches the checker, the mirror no longer raises, and toggling the modes back restores
    the first result bit for bit."""
    from mecano_amd.calculators import ForwardDynamicsCalculator, JointSourceMode, MultiBodyResponseCalculator
    from oracle.cpu_oracle import OracleModel
    torch = torch_cuda
    sys_, desc, locked = make_case("locked2")
    om, B = OracleModel(desc), 70
    q = states(sys_, B)
    fd = ForwardDynamicsCalculator(sys_)
    calc = MultiBodyResponseCalculator(fd)
    joints = sys_.getJointsToConsider()
    bodies = [joints[k].getSuccessor() for k in HUMANOID_TARGETS]
    calc.reset(dev(torch, q))
    first = calc.computeApparentInertiaInverse(bodies).clone()
    fd.setJointSourceModes([int(v) for v in locked])
    calc.reset(dev(torch, q))
    W = calc.computeApparentInertiaInverse(bodies)
    W1 = calc.computeRigidBodyApparentSpatialInertiaInverse(bodies[0])
    torch.cuda.synchronize()
    bounds = ac.bound_of(om, q, desc.n_joints, True)
    ref = ac.apparent_inertia_inverse(om, q, HUMANOID_TARGETS, None, True, locked)
    ac.close_rows(W.cpu().numpy(), ref, bounds, label="locked coupled")
    ac.close_rows(W1.cpu().numpy(), ref[:, :6, :6], bounds, label="locked mirror block")
    assert float((W - first).abs().max()) > 1.0e-3
    fd.setJointSourceModes([JointSourceMode.EFFORT_SOURCE] * desc.n_joints)
    calc.reset(dev(torch, q))
    again = calc.computeApparentInertiaInverse(bodies)
    torch.cuda.synchronize()
    assert torch.equal(again, first)


@pytest.mark.parametrize("case", ["humanoid30", "mixed_tree", "tree128"])
def test_coupled_diagonal_blocks_are_the_diagonal_call_and_W_is_symmetric(torch_cuda, case):
    """COUPLED's diagonal blocks carry DIAGONAL's bits.  Every block is computed (none mirrored), so W = W^T holds to the bound."""
    from oracle.cpu_oracle import OracleModel
    torch = torch_cuda
    sys_, desc, _ = make_case(case)
    hm, om, B, K = model_of(desc, None), OracleModel(desc), 200, 6
    q = states(sys_, B)
    t = targets_of(case, desc, K)
    poses = ac.random_poses(np.random.default_rng(35), K)
    for layout in (AOS, SOA):
        Wc = run(torch, hm, q, t, poses, True, layout)
        Wd = run(torch, hm, q, t, poses, False, layout)
        for k in range(K):
            assert np.array_equal(Wc[:, 6 * k:6 * k + 6, 6 * k:6 * k + 6], Wd[:, k])
        ac.close_rows(Wc, Wc.transpose(0, 2, 1), ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED), label=f"{case} symmetry")


@pytest.mark.parametrize("case", ["humanoid30", "onedof_tree", "mixed_tree"])
def test_mirror_equals_six_forward_dynamics_columns(torch_cuda, case):
    """computeRigidBodyApparentSpatialInertiaInverse / ...LinearInertiaInverse against the route they took before: six mh_aba_bodies_f64
    calls with unit wrenches, computed here."""
    from mecano_amd.calculators import MultiBodyResponseCalculator
    from oracle.cpu_oracle import OracleModel
    torch = torch_cuda
    sys_, desc, _ = make_case(case)
    om, B = OracleModel(desc), 70
    q = states(sys_, B)
    calc = MultiBodyResponseCalculator(sys_)
    calc.reset(dev(torch, q))
    joints = sys_.getJointsToConsider()
    bounds = ac.bound_of(om, q, desc.n_joints, case in WELL_CONDITIONED)
    z = torch.zeros((B, desc.nv), dtype=torch.float64, device="cuda")
    for k in targets_of(case, desc, 3):
        body = joints[k].getSuccessor()
        W = calc.computeRigidBodyApparentSpatialInertiaInverse(body)
        old = torch.empty((B, 6, 6), dtype=torch.float64, device="cuda")
        for c in range(6):
            f = torch.zeros((B, desc.n_joints, 6), dtype=torch.float64, device="cuda")
            f[:, k, c] = 1.0
            old[:, :, c] = calc.model.aba_bodies(dev(torch, q), z, z, (0.0, 0.0, 0.0), f)[1][:, k, :]
        torch.cuda.synchronize()
        ac.close_rows(W.cpu().numpy(), old.cpu().numpy(), bounds, label=f"{case} joint {k}")
        assert torch.equal(calc.computeRigidBodyApparentLinearInertiaInverse(body), W[:, 3:, 3:])
    # numpy in -> numpy out, with a frame
    pose = ac.random_poses(np.random.default_rng(36), 1)[0]
    calc.reset(q)
    Wn = calc.computeRigidBodyApparentSpatialInertiaInverse(joints[0].getSuccessor(), pose)
    assert isinstance(Wn, np.ndarray)
    ac.close_rows(Wn, ac.apparent_inertia_inverse(om, q, [0], pose[None])[:, 0], bounds, label=f"{case} numpy")
    from mecano_amd.multibody import RigidBody
    assert calc.computeRigidBodyApparentSpatialInertiaInverse(RigidBody("stranger")) is None


def test_context_two_streams_and_out_reuse(torch_cuda):
    """A context other than the default one on a stream of its own gives the default context's bits, a second stream too; `out=` is
    written in place and may be used again; after reserve() the call is captured into a graph (it allocates nothing)."""
    torch = torch_cuda
    sys_, desc, _ = make_case("humanoid30")
    hm, B = model_of(desc, None), 1000
    q = dev(torch, states(sys_, B))
    poses = ac.random_poses(np.random.default_rng(37), 4)
    ref = hm.apparent_inertia_inverse(q, HUMANOID_TARGETS, poses, True)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    out = torch.empty_like(ref)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        assert view.apparent_inertia_inverse(q, HUMANOID_TARGETS, poses, True, out=out) is out
        view.check(s1.cuda_stream)
        assert torch.equal(out, ref)
        out.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        view.apparent_inertia_inverse(q, HUMANOID_TARGETS, poses, True, out=out)
        view.check(s2.cuda_stream)
        assert torch.equal(out, ref)
        out.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s2):
            view.apparent_inertia_inverse(q, HUMANOID_TARGETS, poses, True, out=out)
    torch.cuda.synchronize()
    assert not out.any()  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    view.close()


def test_refusals_leave_the_output_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    sys_, desc, _ = make_case("arm7")
    hm, B = model_of(desc, None), 10
    lib = _lib.load()
    q = dev(torch, states(sys_, B))
    W, guard = poisoned(torch, B, (2, 6, 6), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    tgt = np.array([2, 6], dtype=np.int32)
    ident = ac.identity_poses(2)

    def call(fn=lib.mh_apparent_inertia_inverse_f64, B=B, q=q.data_ptr(), n=2, t=tgt.ctypes.data, p=None, blocks=DIAGONAL, out=W.data_ptr()):
        st = fn(hm._h, B, q, n, t, p, blocks, ctypes.byref(opts), out)
        torch.cuda.synchronize()
        return st

    skewed = ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    mirrored = ident.copy()
    mirrored[0, 8] = -1.0
    bad_joint = np.array([2, 7], dtype=np.int32)
    negative = np.array([-1, 2], dtype=np.int32)
    refusals = {"NULL q": dict(q=None), "NULL W_out": dict(out=None), "NULL target_joints": dict(t=None), "no targets": dict(n=0),
                "too many targets": dict(n=17), "joint out of range": dict(t=bad_joint.ctypes.data), "negative joint": dict(t=negative.ctypes.data),
                "unknown blocks": dict(blocks=2), "pose not orthonormal": dict(p=skewed.ctypes.data), "pose a reflection": dict(p=mirrored.ctypes.data),
                "W_out overlaps q": dict(out=q.data_ptr()),
                "W_out overlaps a q inside it": dict(q=W[1].data_ptr())}
    for fn in (lib.mh_apparent_inertia_inverse_f64, lib.mh_apparent_inertia_inverse_f32):
        for what, kw in refusals.items():
            assert call(fn=fn, **kw) == INVALID, what
            assert lib.mh_last_error(), what
            assert "overlaps" not in what or b"overlap" in lib.mh_last_error(), what
            assert torch.isnan(W).all() and torch.isnan(guard).all(), what
    q_before = q.clone()
    assert call(B=0) == 0 and call(B=0, q=None, out=None) == 0
    assert torch.isnan(W).all() and torch.equal(q, q_before)
    assert call(p=ident.ctypes.data) == 0
    assert not torch.isnan(W).any() and torch.isnan(guard).all()
    with pytest.raises(_lib.MecanoHipError):
        hm.apparent_inertia_inverse(q, [1, 2], out=torch.empty((B, 3, 6, 6), dtype=torch.float64, device="cuda"))
    check_bad_outputs(torch, (B, 2, 6, 6), lambda out: hm.apparent_inertia_inverse(q, [1, 2], out=out))
    with pytest.raises(_lib.MecanoHipError):
        hm.apparent_inertia_inverse(q, [1, 2], poses=np.zeros(12))
