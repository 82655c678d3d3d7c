"""mh_body_poses_vjp_* and mh_jacobian_transpose_* on the device against the CPU checker (tests/kinematics_vjp_check.py, pinned by
tests/test_kinematics_vjp_cpu.py) and against the device's own matrices, through the C-ABI (HipModel.body_poses_vjp / jacobian_transpose
are the ctypes calls) and torch.autograd.  Every output is poisoned and has a guard row behind it.

Tolerances, relative to max(1, |ref|_inf) as helpers.close applies them (a gradient sums over up to 16 targets): fp64 1e-10; fp32
helpers.f32_forward_tol(2 n_joints) -- a result is a path of at most n bodies outward and at most n inward."""
import ctypes

import numpy as np
import pytest

import helpers as hp
import kinematics_check as kc
import kinematics_vjp_check as kv
from helpers import DistinctRows, check_bad_outputs, check_cover, close, f32_forward_tol, group_cover, poisoned
from test_gpu_kinematics import AOS, B_MAX, INVALID, SOA, scattered_chains, chains_of, dev, laid_out, model_of
from test_kinematics_cpu import HUMANOID_TARGETS, make_case, states
from test_kinematics_vjp_cpu import cotangents

pytestmark = pytest.mark.gpu

BATCHES = {1: 1, 63: 1, 64: 16, 65: 16, 257: 5}  # batch -> number of targets


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def vjp_chains(case, desc, K):
    """chains_of, with the root body as a target of the K = 5 list of every case (one body is named twice there already)"""
    t, b, poses = chains_of(case, desc, K)
    t, b = list(t), list(b)
    if K == 5 and -1 not in t:
        t[2] = -1
    if K == 5:
        assert -1 in t and len(set(t)) < K
    return t, b, poses


_REFS = {}


def reference(case, K, dtype_name):
    """Inputs and checker results of the first rows of a batch, computed once per (case, K, precision); a smaller batch takes the first
    rows.  fp32: the checker runs in fp64 on the fp32-rounded inputs."""
    key = (case, K, dtype_name)
    if key not in _REFS:
        sys_, desc = make_case(case)
        rows = {1: 64, 16: 65, 5: B_MAX}[K]
        q = states(sys_, desc, rows)[0]
        g, ga, w = cotangents(rows, K, 12, 70 + K), cotangents(rows, desc.n_joints, 12, 71 + K), cotangents(rows, K, 6, 72 + K)
        if dtype_name == "f32":
            q, g, ga, w = (x.astype(np.float32).astype(np.float64) for x in (q, g, ga, w))
        m = kc.KinModel(desc)
        t, b, poses = vjp_chains(case, desc, K)
        _REFS[key] = dict(desc=desc, q=q, g=g, ga=ga, w=w, t=t, b=b, poses=poses, gq=kv.body_poses_vjp(m, q, g, t, poses),
                          gq_all=kv.body_poses_vjp(m, q, ga), tau=kv.jacobian_transpose(m, q, w, t, b, poses))
    return _REFS[key]


def vec_output(torch, B, n, layout, dtype):
    """(tensor to pass as out=, its [B, n] view, guard)"""
    if layout == AOS:
        out, guard = poisoned(torch, B, (n,), dtype)
        return out, out, guard
    out, guard = poisoned(torch, n, (B,), dtype)
    return out, out.t(), guard


def flat(x, layout):
    """[B, K, e] on the device in the call's layout: AoS as it is, SoA [K e, B]"""
    return x if layout == AOS else x.reshape(x.shape[0], -1).t().contiguous()


def tolerance(desc, dtype_name):
    return 1.0e-10 if dtype_name == "f64" else f32_forward_tol(2 * desc.n_joints)


def run_three(torch, hm, desc, B, layout, dtype, q, g, ga, w, t, b, poses):
    """The three calls of a parity check into poisoned outputs: [(label, rows view, guard)]"""
    ql = laid_out(q, layout)
    outs = [vec_output(torch, B, desc.nv, layout, dtype) for _ in range(3)]
    assert hm.body_poses_vjp(ql, flat(g, layout), t, poses, layout, out=outs[0][0]) is outs[0][0]
    hm.body_poses_vjp(ql, flat(ga, layout), None, None, layout, out=outs[1][0])
    hm.jacobian_transpose(ql, flat(w, layout), t, b, poses, layout, out=outs[2][0])
    torch.cuda.synchronize()
    return [(name, o[1], o[2]) for name, o in zip(("body_poses_vjp", "body_poses_vjp of all bodies", "jacobian_transpose"), outs)]


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", ["arm7", "humanoid30", "mixed12"])
def test_matches_checker(torch_cuda, case, layout, dtype_name):
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    hm = None
    for B, K in BATCHES.items():
        R = reference(case, K, dtype_name)
        desc = R["desc"]
        hm = hm or model_of(desc)
        q, g, ga, w = (dev(torch, R[k][:B], dtype) for k in ("q", "g", "ga", "w"))
        got = run_three(torch, hm, desc, B, layout, dtype, q, g, ga, w, R["t"], R["b"], R["poses"])
        for (name, rows, guard), ref in zip(got, (R["gq"], R["gq_all"], R["tau"])):
            check_cover(rows, guard, np.arange(B), ref[:B], tolerance(desc, dtype_name), label=f"{case} B={B} K={K} layout={layout} {dtype_name} {name}")


def _scattered_reference(model, dtype_name):
    """Configurations and cotangents in the identity description's index space and the checker's outputs on them: once per model and
    precision, shared by the layouts, the hole and the re-listing cases, never modified."""
    key = ("scattered", model, dtype_name)
    if key not in _REFS:
        sys_, d0 = hp.SCATTERED_MODELS[model]()
        B = 70
        t, b, poses = vjp_chains("humanoid30", d0, 5) if model == "humanoid30" else scattered_chains(model, d0)
        K = len(t)
        q = DistinctRows(sys_, 16, seed=73).rows(np.arange(B))[0]
        g, ga, w = cotangents(B, K, 12, 74), cotangents(B, d0.n_joints, 12, 75), cotangents(B, K, 6, 76)
        if dtype_name == "f32":
            q, g, ga, w = (x.astype(np.float32).astype(np.float64) for x in (q, g, ga, w))
        m = kc.KinModel(d0)
        _REFS[key] = dict(q=q, g=g, ga=ga, w=w, t=t, b=b, poses=poses, gq=kv.body_poses_vjp(m, q, g, t, poses),
                          gq_all=kv.body_poses_vjp(m, q, ga), tau=kv.jacobian_transpose(m, q, w, t, b, poses))
    return _REFS[key]


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes,relist", [("mixed10", 0, False), ("mixed10", 2, False), ("humanoid30", 0, False), ("humanoid30", 0, True)])
def test_scattered_index_maps(torch_cuda, model, holes, relist, layout, dtype_name):
    """body_poses_vjp (listed targets and every body) and jacobian_transpose on a description whose maps send every DoF and every
    configuration entry somewhere else (with holes: two indices of each space owned by no joint, holding 7.0 in q), against the checker on
    the IDENTITY description under this file's tolerances.  q goes in through the configuration map, the gradients come back through the
    DoF map; the cotangents follow the target list and do not move.  relist: the scattered description's joints are listed in a random
    order, parents possibly after their children -- the joint lists are translated and the cotangents of "every body" follow the new
    listing.  Unowned entries are exact zeros, the guard rows stay poisoned, and read without moving them back the gradients miss the
    reference by more than 1e-3."""
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    R = _scattered_reference(model, dtype_name)
    t, b, order = list(R["t"]), list(R["b"]), np.arange(d0.n_joints)
    if relist:
        d, order = hp.relisted(d, np.random.default_rng(77))
        assert any(d.parent[k] > k for k in range(d.n_joints)) and hp.maps_flags(d) == (0, 1)
        inv = np.argsort(order)
        t, b = [int(inv[j]) if j >= 0 else -1 for j in t], [int(inv[j]) if j >= 0 else -1 for j in b]
    hm, B = hp.scattered_model(d, model) if not relist else model_of(d), 70
    q, g, ga, w = (dev(torch, x, dtype) for x in (hp.to_q(R["q"], pq, d.nq), R["g"], R["ga"][:, order], R["w"]))
    got = run_three(torch, hm, d, B, layout, dtype, q, g, ga, w, t, b, R["poses"])
    for (name, rows, guard), ref in zip(got, (R["gq"], R["gq_all"], R["tau"])):
        label = f"scattered {model} holes={holes} relist={relist} layout={layout} {dtype_name} {name}"
        assert torch.isnan(guard).all(), label + ": wrote past the last row"
        raw = rows.cpu().numpy().astype(np.float64)
        back, free = hp.from_v(raw, pv)
        assert not np.isnan(raw).any() and not free.any(), label  # every entry written, the unowned ones as zeros
        close(back, ref, tolerance(d0, dtype_name), label=label)
        hp.assert_misses(hp.keep_order(raw, pv), ref, label)


def test_tree128_fp32(torch_cuda):
    torch = torch_cuda
    sys_, desc = make_case("tree128")
    hm, m, B = model_of(desc), kc.KinModel(desc), 65
    t, b = [127, 64], [-1, 90]
    poses = kc.random_poses(np.random.default_rng(41), 2)
    q, g, ga, w = (x.astype(np.float32) for x in (states(sys_, desc, B)[0], cotangents(B, 2, 12, 80), cotangents(B, desc.n_joints, 12, 81),
                                                  cotangents(B, 2, 6, 82)))
    q64, g64, ga64, w64 = (x.astype(np.float64) for x in (q, g, ga, w))
    refs = (kv.body_poses_vjp(m, q64, g64, t, poses), kv.body_poses_vjp(m, q64, ga64), kv.jacobian_transpose(m, q64, w64, t, b, poses))
    tol = f32_forward_tol(2 * desc.n_joints)
    for layout in (AOS, SOA):
        got = run_three(torch, hm, desc, B, layout, torch.float32, *(dev(torch, x, torch.float32) for x in (q, g, ga, w)), t, b, poses)
        for (name, rows, guard), ref in zip(got, refs):
            check_cover(rows, guard, np.arange(B), ref, tol, label=f"tree128 layout={layout} {name}")


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_contracts_the_devices_own_matrices(torch_cuda, dtype_name):
    """jacobian_transpose is the einsum of HipModel.geometric_jacobian with the wrenches, body_poses_vjp the same contraction with (n; f)
    formed in torch from HipModel.body_poses: the route the calls replace."""
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    sys_, desc = make_case("humanoid30")
    hm, B, K = model_of(desc), 257, 5
    t, b, poses = vjp_chains("humanoid30", desc, K)
    q = dev(torch, states(sys_, desc, B)[0], dtype)
    g, w = dev(torch, cotangents(B, K, 12, 83), dtype), dev(torch, cotangents(B, K, 6, 84), dtype)
    tol = tolerance(desc, dtype_name)
    J = hm.geometric_jacobian(q, t, b, poses).reshape(B, K, 6, desc.nv)
    close(hm.jacobian_transpose(q, w, t, b, poses).cpu().numpy(), torch.einsum("bkin,bki->bn", J, w).cpu().numpy(), tol, label=f"J^T w {dtype_name}")
    P = hm.body_poses(q, t, poses)
    R, GR = P[..., :9].reshape(B, K, 3, 3), g[..., :9].reshape(B, K, 3, 3)
    M = R.transpose(-1, -2) @ GR
    n = torch.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], dim=-1)
    f = (R.transpose(-1, -2) @ g[..., 9:, None])[..., 0]
    J0 = hm.geometric_jacobian(q, t, None, poses).reshape(B, K, 6, desc.nv)
    ref = torch.einsum("bkin,bki->bn", J0, torch.cat([n, f], dim=-1))
    close(hm.body_poses_vjp(q, g, t, poses).cpu().numpy(), ref.cpu().numpy(), tol, label=f"sum J^T (n; f) {dtype_name}")


def test_exact_zeros(torch_cuda):
    """A zero cotangent, joints on no chain, a list of only the root body and base == target give exact zeros in poisoned outputs."""
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv = model_of(desc), 70, desc.nv
    q = dev(torch, states(sys_, desc, B)[0])
    poses = kc.random_poses(np.random.default_rng(85), 2)
    g, w = dev(torch, cotangents(B, 2, 12, 86)), dev(torch, cotangents(B, 2, 6, 87))

    def run(call, *args):
        out, guard = poisoned(torch, B, (nv,), torch.float64)
        call(*args, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(guard).all() and not torch.isnan(out).any()
        return out

    assert not run(hm.body_poses_vjp, q, torch.zeros_like(g), [2, 5], poses).any()
    assert not run(hm.body_poses_vjp, q, torch.zeros(B, 7, 12, dtype=torch.float64, device="cuda")).any()
    assert not run(hm.jacobian_transpose, q, torch.zeros_like(w), [2, 5], [-1, 3], poses).any()
    gq = run(hm.body_poses_vjp, q, g, [2, 4], poses)  # joints 5 and 6 lie below both targets
    assert not gq[:, 5:].any() and gq[:, :5].abs().amin() > 0
    tau = run(hm.jacobian_transpose, q, w, [2, 5], [-1, 3], poses)  # root -> body 2: joints 0 .. 2; body 3 -> body 5: joints 4, 5
    assert not tau[:, 3].any() and not tau[:, 6].any() and tau[:, [0, 1, 2, 4, 5]].abs().amin() > 0
    tau = run(hm.jacobian_transpose, q, w, [5, 6], [2, 3], poses)  # joints 0 .. 2 lie above both chains: the two seeds meet there
    assert not tau[:, :3].any() and tau[:, 3:].abs().amin() > 0
    assert not run(hm.body_poses_vjp, q, g, [-1, -1], poses).any()
    assert not run(hm.jacobian_transpose, q, w, [-1, -1], None, poses).any()
    assert not run(hm.jacobian_transpose, q, w, [4, -1], [4, -1], poses).any()  # base == target


def test_unowned_dof_indices_get_zeros(torch_cuda):
    """A custom index map with two DoF / configuration indices no joint owns: zeros there, the default map's bits elsewhere."""
    torch = torch_cuda
    sys_, d0 = make_case("arm7")
    B, nv = 70, d0.nv
    q = states(sys_, d0, B)[0]
    place = np.array([k + (k >= 3) + (k >= 5) for k in range(nv)])  # indices 3 and 6 of the wide map stay free
    free = np.setdiff1d(np.arange(nv + 2), place)
    d1 = sys_.toModelDesc()
    d1.dof_indices = place[np.asarray(d0.dof_indices)].astype(np.int32)
    d1.cfg_indices = place[np.asarray(d0.cfg_indices)].astype(np.int32)
    d1.nv = d1.nq = nv + 2
    wide = np.full((B, nv + 2), 0.25)
    wide[:, place] = q
    h0, h1 = model_of(d0), model_of(d1)
    poses = kc.random_poses(np.random.default_rng(88), 2)
    g, w = dev(torch, cotangents(B, 2, 12, 89)), dev(torch, cotangents(B, 2, 6, 90))
    base = (h0.body_poses_vjp(dev(torch, q), g, [2, 6], poses), h0.jacobian_transpose(dev(torch, q), w, [2, 6], [-1, 4], poses))
    for layout in (AOS, SOA):
        outs = [vec_output(torch, B, nv + 2, layout, torch.float64) for _ in range(2)]
        h1.body_poses_vjp(laid_out(dev(torch, wide), layout), flat(g, layout), [2, 6], poses, layout, out=outs[0][0])
        h1.jacobian_transpose(laid_out(dev(torch, wide), layout), flat(w, layout), [2, 6], [-1, 4], poses, layout, out=outs[1][0])
        torch.cuda.synchronize()
        for (_, rows, guard), ref in zip(outs, base):
            assert torch.isnan(guard).all() and not torch.isnan(rows).any()
            assert not rows[:, free].any() and torch.equal(rows[:, place], ref)


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_rows_are_independent(torch_cuda, layout):
    """NaN in one row of q, and in one row of the cotangent: that row is non-finite, every other row has the bits of the clean run."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, K = model_of(desc), 130, 5
    t, b, poses = vjp_chains("humanoid30", desc, K)
    q = dev(torch, states(sys_, desc, B)[0])
    g, ga, w = dev(torch, cotangents(B, K, 12, 91)), dev(torch, cotangents(B, desc.n_joints, 12, 92)), dev(torch, cotangents(B, K, 6, 93))
    clean = run_three(torch, hm, desc, B, layout, torch.float64, q, g, ga, w, t, b, poses)
    bad_q, bad_g, bad_ga, bad_w = q.clone(), g.clone(), ga.clone(), w.clone()
    bad_q[67] = float("nan")
    bad_g[3], bad_ga[3], bad_w[3] = float("nan"), float("nan"), float("nan")
    others = {67: [r for r in range(B) if r != 67], 3: [r for r in range(B) if r != 3]}
    for row, args in ((67, (bad_q, g, ga, w)), (3, (q, bad_g, bad_ga, bad_w))):
        got = run_three(torch, hm, desc, B, layout, torch.float64, *args, t, b, poses)
        for (name, rows, _), (_, ref, _) in zip(got, clean):
            assert not torch.isfinite(rows[row]).all(), f"{name}: row {row} stayed finite"
            assert torch.equal(rows[others[row]], ref[others[row]]), f"{name}: NaN in row {row} reached another row"


_COVER_REFS = {}


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the grid holds (8 per CU), plus a ragged last group: every lane loops over several groups of 64, and its
    workspace -- the wrench accumulators among it -- is used again for the lane's next configuration.  B distinct rows, poisoned outputs
    with guard rows, every row group checked, every entry written."""
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    sys_, desc = make_case("arm7")
    hm, m = model_of(desc), kc.KinModel(desc)
    B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
    rows = DistinctRows(sys_, 256, seed=29)
    q = rows.device(torch, B)[0]
    idx = group_cover(B, grid)
    t, b = [6, 3, 6], [-1, 5, 2]
    poses = kc.random_poses(np.random.default_rng(42), 3)
    g_host, ga_host, w_host = cotangents(64, 3, 12, 94), cotangents(64, desc.n_joints, 12, 95), cotangents(64, 3, 6, 96)
    period = torch.arange(B, device="cuda") % 64
    g, ga, w = (dev(torch, x)[period].contiguous() for x in (g_host, ga_host, w_host))
    got = run_three(torch, hm, desc, B, layout, torch.float64, q, g, ga, w, t, b, poses)
    if B not in _COVER_REFS:  # once for both layouts
        qr = rows.rows(idx)[0]
        _COVER_REFS[B] = (kv.body_poses_vjp(m, qr, g_host[idx % 64], t, poses), kv.body_poses_vjp(m, qr, ga_host[idx % 64]),
                          kv.jacobian_transpose(m, qr, w_host[idx % 64], t, b, poses))
    for (name, out, guard), ref in zip(got, _COVER_REFS[B]):
        check_cover(out, guard, idx, ref, 1.0e-10, label=name)


def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on its own stream gives the default context's bits; after reserve() both calls are captured into one graph, one
    after the other (they allocate nothing), and the replay gives the bits of the direct call, also on changed inputs."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, K = model_of(desc), 1000, 5
    t, b, poses = vjp_chains("humanoid30", desc, K)
    q = dev(torch, states(sys_, desc, B)[0])
    g, w = dev(torch, cotangents(B, K, 12, 97)), dev(torch, cotangents(B, K, 6, 98))
    gq_ref, tau_ref = hm.body_poses_vjp(q, g, t, poses), hm.jacobian_transpose(q, w, t, b, poses)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    gq, tau = torch.zeros_like(gq_ref), torch.zeros_like(tau_ref)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view.body_poses_vjp(q, g, t, poses, out=gq)
        view.jacobian_transpose(q, w, t, b, poses, out=tau)
        view.check(s.cuda_stream)
        assert torch.equal(gq, gq_ref) and torch.equal(tau, tau_ref)
        gq.zero_(), tau.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            view.body_poses_vjp(q, g, t, poses, out=gq)
            view.jacobian_transpose(q, w, t, b, poses, out=tau)
    torch.cuda.synchronize()
    assert not gq.any() and not tau.any()  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gq, gq_ref) and torch.equal(tau, tau_ref)
    q2, g2, w2 = dev(torch, states(sys_, desc, B, seed=6)[0]), dev(torch, cotangents(B, K, 12, 99)), dev(torch, cotangents(B, K, 6, 100))
    gq_ref2, tau_ref2 = hm.body_poses_vjp(q2, g2, t, poses), hm.jacobian_transpose(q2, w2, t, b, poses)
    q.copy_(q2), g.copy_(g2), w.copy_(w2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gq, gq_ref2) and torch.equal(tau, tau_ref2)
    view.close()


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, m, B = model_of(desc), kc.KinModel(desc), 10
    lib = _lib.load()
    q_host = states(sys_, desc, B)[0]
    q = dev(torch, q_host)
    # (one buffer, so that "the output overlaps the cotangent" can name an address inside it)
    g, w = dev(torch, cotangents(B, 2, 12, 101)), dev(torch, cotangents(B, 2, 6, 102))
    out, guard = poisoned(torch, B, (desc.nv,), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    tgt, base = np.array([2, 6], dtype=np.int32), np.array([-1, 4], dtype=np.int32)
    ident = np.tile(kc.IDENTITY12, (2, 1))
    skewed, mirrored = ident.copy(), ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    mirrored[0, 8] = -1.0
    bad_joint, below = np.array([2, 7], dtype=np.int32), np.array([-2, 2], dtype=np.int32)
    q_before, g_before, w_before = q.clone(), g.clone(), w.clone()

    def untouched(what):
        assert lib.mh_last_error(), what
        assert torch.isnan(out).all() and torch.isnan(guard).all(), what
        assert torch.equal(q, q_before) and torch.equal(g, g_before) and torch.equal(w, w_before), what

    def vjp(fn, B=B, q=q.data_ptr(), n=2, t=tgt.ctypes.data, p=None, g=g.data_ptr(), o=out.data_ptr()):
        st = fn(hm._h, B, q, n, t, p, g, ctypes.byref(opts), o)
        torch.cuda.synchronize()
        return st

    def jt(fn, B=B, q=q.data_ptr(), n=2, b=base.ctypes.data, t=tgt.ctypes.data, p=None, w=w.data_ptr(), o=out.data_ptr()):
        st = fn(hm._h, B, q, n, b, t, p, w, ctypes.byref(opts), o)
        torch.cuda.synchronize()
        return st

    common = {"NULL q": dict(q=None), "NULL output": dict(o=None), "no targets": dict(n=0), "too many targets": dict(n=17),
              "target out of range": dict(t=bad_joint.ctypes.data), "target below -1": dict(t=below.ctypes.data),
              "pose not orthonormal": dict(p=skewed.ctypes.data), "pose a reflection": dict(p=mirrored.ctypes.data),
              "output overlaps q": dict(o=q.data_ptr())}
    vjp_refusals = dict(common, **{"NULL g_pose": dict(g=None), "all bodies with another count": dict(t=None, n=2),
                                   "all bodies with poses": dict(t=None, n=7, p=ident.ctypes.data), "output overlaps g_pose": dict(o=g.data_ptr() + 64)})
    jt_refusals = dict(common, **{"NULL wrench": dict(w=None), "NULL target_joints": dict(t=None), "NULL target_joints, every body": dict(t=None, n=7),
                                  "base out of range": dict(b=bad_joint.ctypes.data), "base below -1": dict(b=below.ctypes.data),
                                  "output overlaps wrench": dict(o=w.data_ptr() + 64)})
    for sfx in ("f64", "f32"):
        for what, kw in vjp_refusals.items():
            assert vjp(getattr(lib, "mh_body_poses_vjp_" + sfx), **kw) == INVALID, what
            untouched(what)
        for what, kw in jt_refusals.items():
            assert jt(getattr(lib, "mh_jacobian_transpose_" + sfx), **kw) == INVALID, what
            untouched(what)
    assert vjp(lib.mh_body_poses_vjp_f64, B=0) == 0 and vjp(lib.mh_body_poses_vjp_f64, B=0, q=None, g=None, o=None) == 0
    assert jt(lib.mh_jacobian_transpose_f64, B=0) == 0 and jt(lib.mh_jacobian_transpose_f64, B=0, q=None, w=None, o=None) == 0
    assert torch.isnan(out).all() and torch.isnan(guard).all()
    # the next valid calls are right
    assert vjp(lib.mh_body_poses_vjp_f64, p=ident.ctypes.data) == 0
    assert torch.isnan(guard).all()
    close(out.cpu().numpy(), kv.body_poses_vjp(m, q_host, g.cpu().numpy(), [2, 6]), 1.0e-10, label="after the refusals: body_poses_vjp")
    assert jt(lib.mh_jacobian_transpose_f64, b=None) == 0
    close(out.cpu().numpy(), kv.jacobian_transpose(m, q_host, w.cpu().numpy(), [2, 6]), 1.0e-10, label="after the refusals: jacobian_transpose")
    # the engine's own checks: wrong shapes, and targets=None where there is no all-bodies form
    check_bad_outputs(torch, (B, desc.nv), lambda o: hm.body_poses_vjp(q, g, [2, 6], out=o))
    check_bad_outputs(torch, (B, desc.nv), lambda o: hm.jacobian_transpose(q, w, [2, 6], out=o))
    for call in (lambda: hm.body_poses_vjp(q, g, [1, 2, 3]), lambda: hm.body_poses_vjp(q, w, [2, 6]), lambda: hm.body_poses_vjp(q, g),
                 lambda: hm.jacobian_transpose(q, g, [2, 6]), lambda: hm.jacobian_transpose(q, w, None),
                 lambda: hm.jacobian_transpose(q, w, [2, 6], [1]), lambda: hm.body_poses_vjp(q, g, [2, 6], poses=np.zeros(12)),
                 lambda: hm.body_poses_vjp(q, g, list(range(17)))):
        with pytest.raises(_lib.MecanoHipError):
            call()


@pytest.mark.parametrize("case", ["onedof12", "arm7"])
def test_autograd_backward_is_one_vjp_call(torch_cuda, case):
    """autograd.body_poses(...).backward of a random linear loss is chart_pullback(body_poses_vjp(...)) bit for bit -- onedof12 has a
    floating joint, whose raw quaternion is not of unit length here -- and a second backward raises."""
    from mecano_amd import autograd
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B, K = model_of(desc), 70, 5
    t, _, poses = vjp_chains(case, desc, K)
    q_host = states(sys_, desc, B)[0]
    if case == "onedof12":
        m = kc.KinModel(desc)
        for i in range(m.n):
            if int(m.type[i]) == kc.SIXDOF:
                q_host[:, m.cfgs(i)[:4]] *= 1.25
    c = dev(torch, cotangents(B, K, 12, 103))
    q = dev(torch, q_host).requires_grad_(True)
    P = autograd.body_poses(hm, q, t, poses)
    assert torch.equal(P.detach(), hm.body_poses(q.detach(), t, poses))
    loss = (c * P).sum()
    loss.backward()
    ref = hm.chart_pullback(q.detach(), hm.body_poses_vjp(q.detach(), c, t, poses))
    assert torch.equal(q.grad, ref) and q.grad.abs().amax() > 0.1
    with pytest.raises(RuntimeError):
        loss.backward()
    q_all = dev(torch, q_host).requires_grad_(True)
    ca = dev(torch, cotangents(B, desc.n_joints, 12, 104))
    (ca * autograd.body_poses(hm, q_all)).sum().backward()
    assert torch.equal(q_all.grad, hm.chart_pullback(q_all.detach(), hm.body_poses_vjp(q_all.detach(), ca)))
