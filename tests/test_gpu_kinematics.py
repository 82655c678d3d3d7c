"""mh_body_poses_* and mh_geometric_jacobian_* on the device against the CPU checker (tests/kinematics_check.py, pinned by
tests/test_kinematics_cpu.py), through the C-ABI (HipModel.body_poses / geometric_jacobian are the ctypes calls) and the calculator
mirror.  Every output is poisoned and has a guard row behind it: entries left unwritten and writes past the end show.

Tolerances: fp64 1e-10 absolute (helpers.close); fp32 helpers.f32_forward_tol(n_bodies) times max(1, |ref|_inf), as `close` applies it."""
import ctypes

import numpy as np
import pytest

import helpers as hp
import kinematics_check as kc
from helpers import DistinctRows, check_bad_outputs, check_cover, close, f32_forward_tol, group_cover, poisoned
from test_kinematics_cpu import HUMANOID_TARGETS, make_case, states, targets_of

pytestmark = pytest.mark.gpu

AOS, SOA = 0, 1
INVALID = 1  # MH_ERR_INVALID_ARGUMENT
B_MAX = 257
# batch -> (number of targets, convective term asked for): one ragged wave, one full, one more than full, several; one target, a group of
# five with one body named twice, the full list of sixteen
BATCHES = {1: (1, True), 63: (1, False), 64: (16, True), 65: (16, False), 257: (5, True)}


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def model_of(desc):
    from mecano_amd.engine import HipModel
    return HipModel(desc)


def chains_of(case, desc, K):
    """(targets, bases, poses) of K chains; the humanoid's are its feet and hands, from the root and from a foot"""
    if case == "humanoid30":
        t = (HUMANOID_TARGETS + [12] + [3, 9, 15, 21, 24, 0, 19, 6, 23, 12, 17])[:K] if K > 1 else [19]
        b = ([-1, 6, -1, 19, 6] + [-1, 6, 12, -1, 23, 6, -1, 19, 6, -1, 12])[:K] if K > 1 else [6]
    else:
        t, b = targets_of(case, desc, K)
        if K == 5:
            t[2] = -1  # the root body as a target: its chain climbs from the base only
    return t, b, kc.random_poses(np.random.default_rng(40 + K), K)


_REFS = {}


def reference(case, K, dtype_name):
    """(q, qd, targets, bases, poses, J, conv, target poses, all-body poses) of B_MAX configurations, computed once per (case, K, precision);
    a smaller batch takes the first rows.  fp32: the checker runs in fp64 on the fp32-rounded state."""
    key = (case, K, dtype_name)
    if key not in _REFS:
        sys_, desc = make_case(case)
        rows = {1: 64, 16: 65, 5: B_MAX}.get(K, B_MAX)
        q, qd = states(sys_, desc, rows)
        if dtype_name == "f32":
            q, qd = q.astype(np.float32).astype(np.float64), qd.astype(np.float32).astype(np.float64)
        m = kc.KinModel(desc)
        t, b, poses = chains_of(case, desc, K)
        J, c = kc.geometric_jacobian(m, q, t, b, poses, qd)
        _REFS[key] = dict(desc=desc, q=q, qd=qd, t=t, b=b, poses=poses, J=J, c=c, P=kc.body_poses(m, q, t, poses), P_all=kc.body_poses(m, q))
    return _REFS[key]


def outputs(torch, B, row_shape, layout, dtype):
    """(tensor to pass as out=, its [B, ...] view, guard)"""
    if layout == AOS:
        out, guard = poisoned(torch, B, row_shape, dtype)
        return out, out, guard
    n = int(np.prod(row_shape))
    out, guard = poisoned(torch, n, (B,), dtype)
    return out, out.t(), guard


def laid_out(x, layout):
    return x if layout == AOS else x.t().contiguous()


def tolerance(desc, dtype_name):
    return dict(tol=1.0e-10, absolute=True) if dtype_name == "f64" else dict(tol=f32_forward_tol(desc.n_joints), absolute=False)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", ["arm7", "humanoid30", "mixed12"])
def test_matches_checker(torch_cuda, case, layout, dtype_name):
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    hm = None
    for B, (K, conv) in BATCHES.items():
        R = reference(case, K, dtype_name)
        desc = R["desc"]
        hm = hm or model_of(desc)
        tol = tolerance(desc, dtype_name)
        idx = np.arange(B)
        q, qd = laid_out(dev(torch, R["q"][:B], dtype), layout), laid_out(dev(torch, R["qd"][:B], dtype), layout)
        J, J_rows, J_guard = outputs(torch, B, (6 * K, desc.nv), layout, dtype)
        label = f"{case} B={B} K={K} layout={layout} {dtype_name}"
        if conv:
            c, c_rows, c_guard = outputs(torch, B, (K, 6), layout, dtype)
            hm.geometric_jacobian(q, R["t"], R["b"], R["poses"], qd, True, layout, out=(J, c))
            torch.cuda.synchronize()
            check_cover(c_rows, c_guard, idx, R["c"][:B].reshape(B, -1), label=label + " convective", **tol)
        else:
            assert hm.geometric_jacobian(q, R["t"], R["b"], R["poses"], None, False, layout, out=J) is J
            torch.cuda.synchronize()
        check_cover(J_rows, J_guard, idx, R["J"][:B].reshape(B, -1), label=label + " J", **tol)
        P, P_rows, P_guard = outputs(torch, B, (K, 12), layout, dtype)
        hm.body_poses(q, R["t"], R["poses"], layout, out=P)
        PA, PA_rows, PA_guard = outputs(torch, B, (desc.n_joints, 12), layout, dtype)
        hm.body_poses(q, None, None, layout, out=PA)
        torch.cuda.synchronize()
        check_cover(P_rows, P_guard, idx, R["P"][:B].reshape(B, -1), label=label + " poses", **tol)
        check_cover(PA_rows, PA_guard, idx, R["P_all"][:B].reshape(B, -1), label=label + " poses of all bodies", **tol)


def scattered_chains(model, desc):
    """(targets, bases, poses): the humanoid's five chains of the tests above (one body twice, two from a moving foot); on the mixed tree
    the last body from the root, a body from another branch's body, and the root body from a moving base"""
    if model == "humanoid30":
        return chains_of("humanoid30", desc, 5)
    return [desc.n_joints - 1, 4, -1, 2], [-1, desc.n_joints - 2, 6, -1], kc.random_poses(np.random.default_rng(44), 4)


def _scattered_reference(model, dtype_name):
    """States in the identity description's index space and the checker's outputs on them: once per model and precision, shared by the
    layouts, the hole and the re-listing cases, never modified."""
    key = ("scattered", model, dtype_name)
    if key not in _REFS:
        sys_, d0 = hp.SCATTERED_MODELS[model]()
        q, qd = DistinctRows(sys_, 16, seed=71).rows(np.arange(70), np.float32 if dtype_name == "f32" else np.float64)[:2]
        m = kc.KinModel(d0)
        t, b, poses = scattered_chains(model, d0)
        J, c = kc.geometric_jacobian(m, q, t, b, poses, qd)
        _REFS[key] = dict(q=q, qd=qd, t=t, b=b, poses=poses, J=J, c=c, P=kc.body_poses(m, q, t, poses), P_all=kc.body_poses(m, q))
    return _REFS[key]


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes,relist", [("mixed10", 0, False), ("mixed10", 2, False), ("humanoid30", 0, False), ("humanoid30", 0, True)])
def test_scattered_index_maps(torch_cuda, model, holes, relist, layout, dtype_name):
    """body_poses and geometric_jacobian (with the convective term, chains from the root and from moving bases) on a description whose
    maps send every DoF and every configuration entry somewhere else (with holes: two indices of each space owned by no joint, holding 7.0
    in q and qd), against the checker on the IDENTITY description under this file's tolerances.  Only q, qd and the columns of J move;
    poses and convective terms do not.  relist: the scattered description's joints are listed in a random order, parents possibly after
    their children -- the joint lists are translated, and the poses of "every body" follow the new listing.  The guard rows stay
    poisoned; with its columns left where they are J misses the reference by more than 1e-3, and so do the poses read from q unmoved."""
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    R = _scattered_reference(model, dtype_name)
    t, b, order = list(R["t"]), list(R["b"]), np.arange(d0.n_joints)
    if relist:
        d, order = hp.relisted(d, np.random.default_rng(72))
        assert any(d.parent[k] > k for k in range(d.n_joints)) and hp.maps_flags(d) == (0, 1)
        inv = np.argsort(order)
        t, b = [int(inv[j]) if j >= 0 else -1 for j in t], [int(inv[j]) if j >= 0 else -1 for j in b]
    hm, B, K, nv, n = hp.scattered_model(d, model) if not relist else model_of(d), 70, len(t), d.nv, d0.n_joints
    tol = tolerance(d0, dtype_name)
    idx = np.arange(B)
    q, qd = laid_out(dev(torch, hp.to_q(R["q"], pq, d.nq), dtype), layout), laid_out(dev(torch, hp.to_v(R["qd"], pv, nv), dtype), layout)
    J, J_rows, J_guard = outputs(torch, B, (6 * K, nv), layout, dtype)
    c, c_rows, c_guard = outputs(torch, B, (K, 6), layout, dtype)
    P, P_rows, P_guard = outputs(torch, B, (K, 12), layout, dtype)
    PA, PA_rows, PA_guard = outputs(torch, B, (n, 12), layout, dtype)
    hm.geometric_jacobian(q, t, b, R["poses"], qd, True, layout, out=(J, c))
    hm.body_poses(q, t, R["poses"], layout, out=P)
    hm.body_poses(q, None, None, layout, out=PA)
    torch.cuda.synchronize()
    label = f"scattered {model} holes={holes} relist={relist} layout={layout} {dtype_name}"
    check_cover(c_rows, c_guard, idx, R["c"].reshape(B, -1), label=label + " convective", **tol)
    check_cover(P_rows, P_guard, idx, R["P"].reshape(B, -1), label=label + " poses", **tol)
    check_cover(PA_rows, PA_guard, idx, R["P_all"][:, order].reshape(B, -1), label=label + " poses of all bodies", **tol)
    assert np.isnan(J_guard.cpu().numpy()).all(), label + " J: wrote past the last row"
    J_host = J_rows.cpu().numpy().astype(np.float64).reshape(B, 6 * K, nv)
    J_back, _ = hp.from_cols(J_host, pv)
    assert not np.isnan(J_back).any(), label + " J: owned columns left unwritten"
    close(J_back, R["J"], label=label + " J", **tol)
    hp.assert_misses(hp.keep_order(J_host, pv), R["J"], "J, columns left where they are")
    if not holes:  # the same description fed q as the identity description lists it: the poses must notice
        hm.body_poses(laid_out(dev(torch, R["q"], dtype), layout), t, R["poses"], layout, out=P)
        torch.cuda.synchronize()
        hp.assert_misses(P_rows.cpu().numpy().astype(np.float64).reshape(B, K, 12), R["P"], "poses from q unmoved")


def test_tree128_fp32(torch_cuda):
    torch = torch_cuda
    sys_, desc = make_case("tree128")
    hm, m, B = model_of(desc), kc.KinModel(desc), 65
    q, qd = (x.astype(np.float32) for x in states(sys_, desc, B))
    t, b = [127, 64], [-1, 90]
    poses = kc.random_poses(np.random.default_rng(41), 2)
    J_ref, c_ref = kc.geometric_jacobian(m, q.astype(np.float64), t, b, poses, qd.astype(np.float64))
    tol = f32_forward_tol(desc.n_joints)
    for layout in (AOS, SOA):
        J, J_rows, J_guard = outputs(torch, B, (12, desc.nv), layout, torch.float32)
        c, c_rows, c_guard = outputs(torch, B, (2, 6), layout, torch.float32)
        hm.geometric_jacobian(laid_out(dev(torch, q, torch.float32), layout), t, b, poses, laid_out(dev(torch, qd, torch.float32), layout), True, layout,
                              out=(J, c))
        P, P_rows, P_guard = outputs(torch, B, (desc.n_joints, 12), layout, torch.float32)
        hm.body_poses(laid_out(dev(torch, q, torch.float32), layout), layout=layout, out=P)
        torch.cuda.synchronize()
        check_cover(J_rows, J_guard, np.arange(B), J_ref.reshape(B, -1), tol, label=f"tree128 J layout={layout}")
        check_cover(c_rows, c_guard, np.arange(B), c_ref.reshape(B, -1), tol, label=f"tree128 convective layout={layout}")
        check_cover(P_rows, P_guard, np.arange(B), kc.body_poses(m, q.astype(np.float64)).reshape(B, -1), tol, label=f"tree128 poses layout={layout}")


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the grid holds (8 per CU), plus a ragged last group: every lane loops over several groups of 64.  B
    distinct rows, poisoned outputs with guard rows, every row group checked, every entry written."""
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    sys_, desc = make_case("arm7")
    hm, m = model_of(desc), kc.KinModel(desc)
    B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
    rows = DistinctRows(sys_, 256, seed=29)
    q, qd = rows.device(torch, B)[:2]
    idx = group_cover(B, grid)
    t, b = [6, 3, 6], [-1, 5, 2]
    poses = kc.random_poses(np.random.default_rng(42), 3)
    J, J_rows, J_guard = outputs(torch, B, (18, desc.nv), layout, torch.float64)
    c, c_rows, c_guard = outputs(torch, B, (3, 6), layout, torch.float64)
    P, P_rows, P_guard = outputs(torch, B, (desc.n_joints, 12), layout, torch.float64)
    hm.geometric_jacobian(laid_out(q, layout), t, b, poses, laid_out(qd, layout), True, layout, out=(J, c))
    hm.body_poses(laid_out(q, layout), layout=layout, out=P)
    torch.cuda.synchronize()
    qr, qdr = rows.rows(idx)[:2]
    J_ref, c_ref = kc.geometric_jacobian(m, qr, t, b, poses, qdr)
    check_cover(J_rows, J_guard, idx, J_ref.reshape(len(idx), -1), 1.0e-10, True, label="J")
    check_cover(c_rows, c_guard, idx, c_ref.reshape(len(idx), -1), 1.0e-10, True, label="convective")
    check_cover(P_rows, P_guard, idx, kc.body_poses(m, qr).reshape(len(idx), -1), 1.0e-10, True, label="poses")


def test_zero_columns_are_written_and_locked_joints_change_nothing(torch_cuda):
    """Columns of joints off the chain are exact zeros in a poisoned output, and a model with acceleration-source joints gives the bits of
    the plain one: kinematics does not know the source modes."""
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B = model_of(desc), 70
    q = dev(torch, states(sys_, desc, B)[0])
    J, guard = poisoned(torch, B, (12, desc.nv), torch.float64)
    hm.geometric_jacobian(q, [2, 5], [-1, 3], out=J)
    torch.cuda.synchronize()
    assert torch.isnan(guard).all() and not torch.isnan(J).any()
    assert not J[:, :6, 3:].any() and J[:, :6, :3].abs().amax() > 0.1  # root -> body 2: joints 0 .. 2
    assert not J[:, 6:, :4].any() and not J[:, 6:, 6:].any() and J[:, 6:, 4:6].abs().amax() > 0.1  # body 3 -> body 5: joints 4, 5
    locked = model_of(desc)
    modes = np.zeros(desc.n_joints, dtype=np.int32)
    modes[[1, 4]] = 1
    locked.set_joint_source_modes(modes)
    assert torch.equal(locked.geometric_jacobian(q, [2, 5], [-1, 3]), J)
    assert torch.equal(locked.body_poses(q), hm.body_poses(q))


def test_stacked_jacobian_gives_the_coupled_apparent_inertia(torch_cuda):
    """With every base at the root the stacked matrix is the J of MH_APPARENT_BLOCKS_COUPLED: J H^-1 J^T on the device against
    mh_apparent_inertia_inverse_f64.  cond_inf(H) <= 420 on the humanoid: the standing 1e-10."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = model_of(desc), 70
    q = dev(torch, states(sys_, desc, B)[0])
    poses = kc.random_poses(np.random.default_rng(43), 4)
    J = hm.geometric_jacobian(q, HUMANOID_TARGETS, None, poses)
    W = J @ hm.mass_matrix_inverse(q) @ J.transpose(1, 2)
    ref = hm.apparent_inertia_inverse(q, HUMANOID_TARGETS, poses, True)
    torch.cuda.synchronize()
    close(W.cpu().numpy(), ref.cpu().numpy(), 1.0e-10, True, label="J Hinv J^T")


def test_context_second_stream_and_graph_capture(torch_cuda):
    """A context of its own on a second stream gives the default context's bits, and after reserve() the calls are captured into a graph
    (they allocate nothing) that replays to the same bits."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = model_of(desc), 1000
    q, qd = (dev(torch, x) for x in states(sys_, desc, B))
    t, b, poses = chains_of("humanoid30", desc, 5)
    J_ref, c_ref = hm.geometric_jacobian(q, t, b, poses, qd, True)
    P_ref = hm.body_poses(q, t, poses)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    J, c, P = torch.zeros_like(J_ref), torch.zeros_like(c_ref), torch.zeros_like(P_ref)
    s2 = torch.cuda.Stream()
    with torch.cuda.stream(s2):
        view.geometric_jacobian(q, t, b, poses, qd, True, out=(J, c))
        view.body_poses(q, t, poses, out=P)
        view.check(s2.cuda_stream)
        assert torch.equal(J, J_ref) and torch.equal(c, c_ref) and torch.equal(P, P_ref)
        J.zero_(), c.zero_(), P.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s2):
            view.geometric_jacobian(q, t, b, poses, qd, True, out=(J, c))
            view.body_poses(q, t, poses, out=P)
    torch.cuda.synchronize()
    assert not J.any() and not P.any()  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(J, J_ref) and torch.equal(c, c_ref) and torch.equal(P, P_ref)
    view.close()


def test_calculator_mirror(torch_cuda):
    """GeometricJacobianCalculator: the compact matrix in base-to-end-effector joint order, the convective term, twist, acceleration and
    joint torques, foot to hand across the common ancestor, against the checker."""
    from mecano_amd.calculators import GeometricJacobianCalculator
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    m, B = kc.KinModel(desc), 70
    q, qd = states(sys_, desc, B)
    joints = sys_.getJointsToConsider()
    calc = GeometricJacobianCalculator(sys_)
    calc.setKinematicChain(joints[6].getSuccessor(), joints[19].getSuccessor())
    pose = kc.random_poses(np.random.default_rng(44), 1)[0]
    calc.setJacobianFrame(pose)
    calc.reset(dev(torch, q), dev(torch, qd))
    Jc = calc.getJacobianMatrix()
    cv = calc.getConvectiveTermMatrix()
    chain = calc.getJointsFromBaseToEndEffector()
    assert [j.getName() for j in chain] == [joints[k].getName() for k, _ in kc.joint_chain(m, 6, 19)]
    assert calc.getNumberOfDegreesOfFreedom() == Jc.shape[2] == sum(j.getDegreesOfFreedom() for j in chain)
    qc = torch.tensor(np.random.default_rng(45).uniform(-1, 1, (B, Jc.shape[2])), device="cuda")
    w = torch.tensor(np.random.default_rng(46).uniform(-1, 1, (B, 6)), device="cuda")
    twist, acc, tau = calc.getEndEffectorTwist(qc), calc.getEndEffectorAcceleration(qc), calc.getJointTorques(w)
    torch.cuda.synchronize()
    for r in range(0, B, 9):
        T0 = kc.joint_frames(m, q[r])
        ch, J_ref = kc.compact_jacobian(m, T0, 6, 19, pose)
        close(Jc[r].cpu().numpy(), J_ref, 1.0e-10, True, label="compact J")
        close(cv[r].cpu().numpy(), kc.convective_term(m, ch, J_ref, qd[r]), 1.0e-10, True, label="convective term")
        close(twist[r].cpu().numpy(), J_ref @ qc[r].cpu().numpy(), 1.0e-10, True, label="twist")
        close(acc[r].cpu().numpy(), J_ref @ qc[r].cpu().numpy() + cv[r].cpu().numpy(), 1.0e-10, True, label="acceleration")
        close(tau[r].cpu().numpy(), J_ref.T @ w[r].cpu().numpy(), 1.0e-10, True, label="joint torques")
    with pytest.raises(ValueError):
        calc.setJacobianFrame(joints[3].getSuccessor())  # a frame that is not fixed in the end effector


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B = model_of(desc), 10
    lib = _lib.load()
    q, qd = (dev(torch, x) for x in states(sys_, desc, B))
    J, J_guard = poisoned(torch, B, (12, desc.nv), torch.float64)
    c, c_guard = poisoned(torch, B, (2, 6), torch.float64)
    P, P_guard = poisoned(torch, B, (7, 12), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    tgt, base = np.array([2, 6], dtype=np.int32), np.array([-1, 4], dtype=np.int32)
    ident = np.tile(kc.IDENTITY12, (2, 1))
    skewed, mirrored = ident.copy(), ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    mirrored[0, 8] = -1.0
    bad_joint, below = np.array([2, 7], dtype=np.int32), np.array([-2, 2], dtype=np.int32)

    def untouched(what):
        assert lib.mh_last_error(), what
        for t in (J, J_guard, c, c_guard, P, P_guard):
            assert torch.isnan(t).all(), what

    def jac(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), n=2, b=base.ctypes.data, t=tgt.ctypes.data, p=None, J=J.data_ptr(), c=c.data_ptr()):
        st = fn(hm._h, B, q, qd, n, b, t, p, ctypes.byref(opts), J, c)
        torch.cuda.synchronize()
        return st

    def pos(fn, B=B, q=q.data_ptr(), n=2, t=tgt.ctypes.data, p=None, out=P.data_ptr()):
        st = fn(hm._h, B, q, n, t, p, ctypes.byref(opts), out)
        torch.cuda.synchronize()
        return st

    jac_refusals = {"NULL q": dict(q=None), "NULL J_out": dict(J=None), "NULL target_joints": dict(t=None), "no targets": dict(n=0),
                    "too many targets": dict(n=17), "target out of range": dict(t=bad_joint.ctypes.data), "target below -1": dict(t=below.ctypes.data),
                    "base out of range": dict(b=bad_joint.ctypes.data), "base below -1": dict(b=below.ctypes.data),
                    "pose not orthonormal": dict(p=skewed.ctypes.data), "pose a reflection": dict(p=mirrored.ctypes.data),
                    "conv_out without qd": dict(qd=None), "J_out overlaps q": dict(J=q.data_ptr()), "conv_out overlaps qd": dict(c=qd.data_ptr()),
                    "conv_out overlaps J_out": dict(c=J.data_ptr() + 64), "J_out overlaps qd": dict(J=qd.data_ptr())}
    pos_refusals = {"NULL q": dict(q=None), "NULL pose_out": dict(out=None), "no targets": dict(n=0), "too many targets": dict(n=17),
                    "all bodies with another count": dict(t=None, n=2), "all bodies with poses": dict(t=None, n=7, p=ident.ctypes.data),
                    "target out of range": dict(t=bad_joint.ctypes.data), "target below -1": dict(t=below.ctypes.data),
                    "pose not orthonormal": dict(p=skewed.ctypes.data), "pose a reflection": dict(p=mirrored.ctypes.data),
                    "pose_out overlaps q": dict(out=q.data_ptr())}
    for sfx in ("f64", "f32"):
        for what, kw in jac_refusals.items():
            assert jac(getattr(lib, "mh_geometric_jacobian_" + sfx), **kw) == INVALID, what
            untouched(what)
        for what, kw in pos_refusals.items():
            assert pos(getattr(lib, "mh_body_poses_" + sfx), **kw) == INVALID, what
            untouched(what)
    q_before = q.clone()
    assert jac(lib.mh_geometric_jacobian_f64, B=0) == 0 and jac(lib.mh_geometric_jacobian_f64, B=0, q=None, J=None, c=None) == 0
    assert pos(lib.mh_body_poses_f64, B=0) == 0 and pos(lib.mh_body_poses_f64, B=0, q=None, out=None) == 0
    untouched("B = 0")
    assert torch.equal(q, q_before)
    assert jac(lib.mh_geometric_jacobian_f64, qd=None, c=None) == 0  # qd may be NULL without the convective term
    assert jac(lib.mh_geometric_jacobian_f64, p=ident.ctypes.data) == 0 and pos(lib.mh_body_poses_f64, t=None, n=7) == 0
    for t, g in ((J, J_guard), (c, c_guard), (P, P_guard)):
        assert not torch.isnan(t).any() and torch.isnan(g).all()
    with pytest.raises(_lib.MecanoHipError):
        hm.geometric_jacobian(q, [1, 2], out=torch.empty((B, 6, desc.nv), dtype=torch.float64, device="cuda"))
    check_bad_outputs(torch, (B, 12, desc.nv), lambda out: hm.geometric_jacobian(q, [1, 2], out=out))
    check_bad_outputs(torch, [(B, 12, desc.nv), (B, 2, 6)], lambda out: hm.geometric_jacobian(q, [1, 2], qd=qd, convective=True, out=out))
    check_bad_outputs(torch, (B, 2, 12), lambda out: hm.body_poses(q, [1, 2], out=out))
    with pytest.raises(_lib.MecanoHipError):
        hm.body_poses(q, [1, 2], poses=np.zeros(12))
    with pytest.raises(_lib.MecanoHipError):
        hm.geometric_jacobian(q, [1, 2], convective=True)
