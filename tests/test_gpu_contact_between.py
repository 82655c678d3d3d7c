"""mh_contact_impulse_between_* on the device against the CPU checker running the same sweeps on the relative terms
(tests/contact_between_check.py, pinned by tests/test_contact_between_cpu.py), through the C-ABI (HipModel.contact_impulse_between is the
ctypes call).  Every output is poisoned and has a guard row behind it: entries left unwritten and writes past the end show.

Parity bound: helpers.close_aba on (qd_next, impulse) with cond_inf of the KKT matrix of the stick system between the same bodies -- the
bound of tests/test_gpu_contact_dynamics.py -- beside the momentum balance H (qd_out - qd) = J_rel^T impulse through the checker's H and
relative J with cond_inf(H), exact zeros in the rows that take no part, and residual_out to the same bound.  corners_k8 in fp32, whose
cond_inf(KKT) u exceeds 1, is held after 1 and 3 sweeps from a stale start under cond_inf(H) instead.
tests/test_contact_between_cpu.py::test_planted_faults_are_rejected_by_the_comparisons_of_the_device_tests holds these very comparisons
against an unloaded base, a base loaded with the wrong sign, rooted S, a rooted b and a neighbour's Z."""
import ctypes

import numpy as np
import pytest

import contact_dynamics_check as cd
import helpers as hp
import kinematics_check as kc
import relative_constraints_check as rc
from helpers import DistinctRows, U32, check_cover, close_aba, f32_aba_forward_factor, f32_forward_tol, group_cover, poisoned
from test_contact_between_cpu import (AT_REST, BLOCK_A, BLOCK_B, BLOCK_NORMAL, CASES, CONVERGED_CASES, block_closed_form, block_collisions, make_inputs,
                                      model_of, momentum_balance, solve, stick_inside, two_blocks)
from test_contact_dynamics_cpu import held_to_H, held_to_kkt, mixed_mu, stale_start
from test_gpu_constrained_dynamics import (AOS, B_MAX, BATCHES, INVALID, SOA, U64, dev, hip_model, laid_out, moved_inputs, outputs,
                                           scattered_description, torch_cuda)  # noqa: F401
from test_gpu_contact_dynamics import device_inputs, set_path, three_outputs

pytestmark = pytest.mark.gpu

_REFS = {}


def reference(name, dtype_name):
    """(inputs, checker result) of B_MAX configurations with mixed_mu, random active and v_normal, once per (case, precision)"""
    key = (name, dtype_name)
    if key not in _REFS:
        I = make_inputs(name, B_MAX, seed=1, dtype=np.float64 if dtype_name == "f64" else np.float32)
        _REFS[key] = (I, solve(name, I, mixed_mu(len(I["targets"])), None, I["active"], I["v_normal"]))
    return _REFS[key]


def call(hm, D, I, mu, sweeps, layout, out=None, init=None, active=True, v_normal=True, bases="own"):
    K = len(I["targets"])
    return hm.contact_impulse_between(D["q"], D["qd"], I["targets"], I["bases"] if isinstance(bases, str) else bases, [mu] * K if np.isscalar(mu) else mu,
                                      I["poses"], D["normals"], D["active"] if active else None, D["v_normal"] if v_normal else None, I["compliance"],
                                      sweeps, init, layout, out)


def read(rows, B, K=None):
    x = rows.cpu().numpy().astype(np.float64)
    return x if K is None else x.reshape(B, K, 6)


# (corners_k8 in fp32: cond_inf(KKT) u > 1, the bound holds nothing there -- test_corners_k8 holds it after few sweeps under cond_inf(H))
@pytest.mark.parametrize("name,dtype_name", [(name, d) for name in CASES for d in ("f64", "f32") if (name, d) != ("corners_k8", "f32")])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_matches_checker(torch_cuda, name, layout, dtype_name):
    torch = torch_cuda
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R = reference(name, dtype_name)
    _, desc, om = model_of(name)
    hm = hip_model(desc)
    K, n = len(I["targets"]), desc.n_joints
    mu = mixed_mu(K)
    for B in BATCHES:
        label = f"between {name} B={B} layout={layout} {dtype_name}"
        rows = slice(0, B)
        D = device_inputs(torch, I, B, layout, dtype)
        (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, K, layout, dtype)
        call(hm, D, I, mu, I["sweeps"], layout, (qdn, imp, res))
        torch.cuda.synchronize()
        assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
        v, p, r = read(qdn_rows, B), read(imp_rows, B, K), read(res_rows, B)
        assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
        assert not p[:, :, :3].any(), label + ": an angular row is not exactly zero"
        assert not p[I["active"][:B] == 0].any(), label + ": an open contact has an impulse"
        print(f"{label}: |qd+ - ref| = {np.abs(v - R['qd_next'][:B]).max():.3e}, |impulse - ref| = {np.abs(p - R['impulse'][:B]).max():.3e}, "
              f"|residual - ref| = {np.abs(r - R['residual'][:B]).max():.3e}, cond_kkt <= {R['cond_kkt'][:B].max():.2e}")
        held_to_kkt(v, p, R, rows, n, u, label)
        close_aba(r[:, None], R["residual"][:B, None], None, n, u, label=label + " residual", conds=R["cond_kkt"][:B])
        momentum_balance(v, p, I, R, rows, n, u, label)
    assert np.abs(R["impulse"]).max() > 0.1


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("holes,relist", [(0, False), (0, True), (2, False)])
def test_scattered_index_maps(torch_cuda, holes, relist, layout, dtype_name):
    """mixed_k3 of test_matches_checker (a rooted contact, two between moving bodies) on maps that send every DoF and every configuration
    entry of the humanoid somewhere else (also with two indices of each space owned by no joint, holding 7.0 in q and qd, and with its
    joints re-listed and both joint lists translated), against ITS reference -- the checker on the identity description -- under its
    bound: held_to_kkt and close_aba on the residual.  Both forms of the solve, S resident in LDS and S streamed, each forced.  q and qd go
    in through the maps, qd+ comes back through the DoF map; impulses and residuals do not move.  Guard rows stay poisoned; read without
    moving it back qd+ misses the reference by more than 1e-3."""
    torch = torch_cuda
    name = "mixed_k3"
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R = reference(name, dtype_name)
    _, desc, om = model_of(name)
    d, pv, pq, targets, bases, order = scattered_description(name, desc, holes, relist, I["targets"], I["bases"])
    hm = hip_model(d)
    assert relist or hm.kernel_variant.startswith("topo:"), hm.kernel_variant
    B, K, n, nv = 70, len(targets), desc.n_joints, d.nv
    D = moved_inputs(torch, I, B, pv, pq, d, order, layout, dtype, keys=("q", "qd", "normals", "v_normal"))
    J, rows = dict(I, targets=targets, bases=bases), slice(0, B)
    try:
        for path in (1, 0):
            label = f"between scattered holes={holes} relist={relist} path={path} layout={layout} {dtype_name}"
            set_path(hm, path)
            (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, nv, K, layout, dtype)
            call(hm, D, J, mixed_mu(K), I["sweeps"], layout, (qdn, imp, res))
            torch.cuda.synchronize()
            assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
            raw, p, r = read(qdn_rows, B), read(imp_rows, B, K), read(res_rows, B)
            v = hp.from_v(raw, pv)[0]
            assert np.all(hp.from_v(raw, pv)[1] == hp.UNOWNED), label + ": entries of qd_out no joint owns do not hold those of qd"
            assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
            assert not p[:, :, :3].any() and not p[I["active"][:B] == 0].any(), label
            held_to_kkt(v, p, R, rows, n, u, label)
            close_aba(r[:, None], R["residual"][:B, None], None, n, u, label=label + " residual", conds=R["cond_kkt"][:B])
            hp.assert_misses(hp.keep_order(raw, pv), R["qd_next"][:B], label + " qd+")
    finally:
        set_path(hm, -1)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_corners_k8(torch_cuda, layout, dtype_name):
    """n_app = 16, S singular, the streamed path in fp64.  fp64: 20 sweeps under cond_inf(KKT) (test_matches_checker); here fp64 and fp32
    after 1 and 3 sweeps from stale_start under cond_inf(H), with the momentum balance."""
    torch = torch_cuda
    name = "corners_k8"
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    _, desc, om = model_of(name)
    hm, B, K, n = hip_model(desc), 65, 8, desc.n_joints
    I = make_inputs(name, B, seed=1, dtype=np.float64 if dtype_name == "f64" else np.float32)
    start = stale_start(I)
    D = device_inputs(torch, I, B, layout, dtype)
    init = laid_out(dev(torch, start, dtype), layout)
    for sweeps in (1, 3):
        label = f"between {name} {sweeps} sweeps layout={layout} {dtype_name}"
        R = solve(name, I, mixed_mu(K), sweeps, I["active"], I["v_normal"], start)
        (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, K, layout, dtype)
        call(hm, D, I, mixed_mu(K), sweeps, layout, (qdn, imp, res), init=init)
        torch.cuda.synchronize()
        assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
        v, p, r = read(qdn_rows, B), read(imp_rows, B, K), read(res_rows, B)
        assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
        assert not p[:, :, :3].any() and not p[I["active"] == 0].any(), label + ": a row that takes no part is not exactly zero"
        held_to_H(p, R, slice(0, B), n, u, label)
        momentum_balance(v, p, I, R, slice(0, B), n, u, label)
        assert np.abs(R["impulse"]).max() > 0.1


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_root_bases_give_the_bits_of_the_rooted_call(torch_cuda, layout, dtype_name):
    torch = torch_cuda
    name = "pairs_k4"
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 65
    I = make_inputs(name, B, seed=2, dtype=np.float64 if dtype_name == "f64" else np.float32)
    mu = mixed_mu(4)
    D = device_inputs(torch, I, B, layout, dtype)
    want = hm.contact_impulse(D["q"], D["qd"], I["targets"], mu, I["poses"], D["normals"], D["active"], D["v_normal"], 1.0e-3, 30, None, layout)
    moving = [t.clone() for t in call(hm, D, I, mu, 30, layout)]  # (a relative call in between: the scratch it leaves behind changes nothing)
    for bases in ([-1] * 4, None):
        got = hm.contact_impulse_between(D["q"], D["qd"], I["targets"], bases, mu, I["poses"], D["normals"], D["active"], D["v_normal"], 1.0e-3, 30, None, layout)
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g, w), f"layout={layout} {dtype_name} bases={bases}"
    assert want[1].any() and not torch.equal(moving[1], want[1])


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_two_blocks_collide_as_the_closed_form_says(torch_cuda, dtype_name):
    """The collision of tests/test_contact_between_cpu.py on the device, 64 velocity pairs and restitutions for each of four mass ratios
    (a model holds one mass per body): the closed-form impulse and velocities, and the total momentum unchanged."""
    torch = torch_cuda
    dtype, tol = (torch.float64, 1.0e-12) if dtype_name == "f64" else (torch.float32, f32_forward_tol(2))
    B = 64
    m_a, m_b, q, qd, e = block_collisions(B)
    rnd = lambda x: np.asarray(x).astype(np.float32 if dtype_name == "f32" else np.float64).astype(np.float64)
    q, qd = rnd(q), rnd(qd)
    v_n = rnd(e * (qd[:, 0] - qd[:, 1]))  # -e u_n
    for ma, mb in ((1.0, 1.0), (0.1, 7.0), (9.0, 0.3), (2.5, 4.0)):
        _, desc = two_blocks(ma, mb)
        hm = hip_model(desc)
        e_eff = v_n / (qd[:, 0] - qd[:, 1])
        want_lam, want_qd = block_closed_form(np.full(B, ma), np.full(B, mb), qd, e_eff)
        nh = dev(torch, np.tile(BLOCK_NORMAL, (B, 1, 1)), dtype)
        qdn, imp, res = hm.contact_impulse_between(dev(torch, q, dtype), dev(torch, qd, dtype), [BLOCK_A], [BLOCK_B], [0.0], None, nh,
                                                   None, dev(torch, v_n[:, None], dtype), 0.0, 50)
        torch.cuda.synchronize()
        v, p = read(qdn, B), read(imp, B, 1)
        label = f"two blocks {ma} : {mb} {dtype_name}"
        print(f"{label}: |lam - closed form| = {np.abs(p[:, 0, 3:] - want_lam[:, None] * BLOCK_NORMAL).max():.2e}, |qd+ - closed form| = {np.abs(v - want_qd).max():.2e}")
        assert np.abs(p[:, 0, 3:] - want_lam[:, None] * BLOCK_NORMAL).max() <= tol * max(1.0, np.abs(want_lam).max()), label
        assert np.abs(v - want_qd).max() <= tol * max(1.0, np.abs(want_qd).max()), label
        p0, p1 = ma * qd[:, 0] + mb * qd[:, 1], ma * v[:, 0] + mb * v[:, 1]
        assert np.abs(p1 - p0).max() <= tol * max(1.0, np.abs(p0).max()), label + ": momentum"
        assert not p[:, :, :3].any() and np.abs(want_lam).min() > 0.0


@pytest.mark.parametrize("name,mu", [("hands_k1", 0.0), ("hands_k1", 100.0), ("mixed_k3", 0.0), ("mixed_k3", 0.5), ("mixed_k3", 100.0)])
def test_converged_impulses_solve_the_contact_problem(torch_cuda, name, mu):
    """1000 sweeps in fp64, every contact closed: the natural residual of the device's impulses through the checker's relative S and b
    vanishes (mu = 0 and 0.5), they lie in their cones, at mu = 0 they are the enumerated complementarity solution, and at mu = 100 the
    configurations whose stick solution lies inside its cone -- and whose sweeps have come to rest, AT_REST of
    tests/test_contact_between_cpu.py, read from the CHECKER's residual -- give the impulses of
    HipModel.constraint_impulse(..., bases=...) with point rows."""
    torch = torch_cuda
    assert name in CONVERGED_CASES
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 64
    I = make_inputs(name, B)
    K = len(I["targets"])
    D = device_inputs(torch, I, B, AOS, torch.float64)
    _, imp, res = call(hm, D, I, mu, 1000, AOS, active=False, v_normal=False)
    torch.cuda.synchronize()
    lam = imp.cpu().numpy()[:, :, 3:]
    R = solve(name, I, mu, 1000)
    scale = max(1.0, np.abs(lam).max())
    nat = cd.natural_residual(R["S"], R["b"], R["n"], [mu] * K, None, I["compliance"], lam)
    print(f"between {name} mu={mu}: natural residual {nat.max():.2e}, |lam| <= {scale:.2f}, residual_out <= {float(res.max()):.2e}")
    ln = np.einsum("bki,bki->bk", R["n"], lam)
    lt = np.linalg.norm(lam - ln[:, :, None] * R["n"], axis=2)
    assert ln.min() >= -1.0e-12 * scale and (lt <= mu * ln + 1.0e-12 * scale).all() and np.abs(lam).max() > 0.1
    if mu < 100.0:
        assert nat.max() <= 1.0e-9 * scale
    if mu == 0.0:
        assert np.abs(lam - cd.frictionless_exact(R["S"], R["b"], R["n"], None, I["compliance"])).max() <= 1.0e-9 * scale
    if mu == 100.0:
        _, stick = hm.constraint_impulse(D["q"], D["qd"], I["targets"], [rc.POINT] * K, I["poses"], bases=I["bases"])
        ls = stick.cpu().numpy()[:, :, 3:]
        inside = stick_inside(R["n"], ls, mu) & (R["residual"] <= AT_REST)
        assert inside.sum() * 4 >= B
        assert np.abs(lam[inside] - ls[inside]).max() <= 1.0e-9 * max(1.0, np.abs(ls[inside]).max())


@pytest.mark.parametrize("name,dtype_name", [("mixed_k3", "f64"), ("mixed_k6", "f64"), ("corners_k8", "f32"), ("hands_k1", "f32")])
def test_resident_and_streamed_solves_give_the_same_bits(torch_cuda, name, dtype_name):
    """S in LDS (copied after the reduction of W) against the reduced W streamed from scratch, each forced."""
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 200
    I = make_inputs(name, B, seed=2, dtype=np.float64 if dtype_name == "f64" else np.float32)
    mu = mixed_mu(len(I["targets"]))
    for layout in (AOS, SOA):
        D = device_inputs(torch, I, B, layout, dtype)
        got = []
        for path in (1, 0, -1):
            set_path(hm, path)
            got.append([t.clone() for t in call(hm, D, I, mu, 30, layout)])
        torch.cuda.synchronize()
        assert got[0][1].any()
        for a, b, c in zip(*got):
            assert torch.equal(a, b) and torch.equal(a, c), f"between {name} {dtype_name} layout={layout}: the two paths differ"
    set_path(hm, -1)


_COVER = {}


def cover_reference(torch):
    if not _COVER:
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        sys_, desc, om = model_of("mixed_k3")
        _, targets, bases, _, _ = CASES["mixed_k3"]
        B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
        rows = DistinctRows(sys_, 256, seed=43)
        idx = group_cover(B, grid)
        q, qd, _, _ = rows.rows(idx)
        poses = kc.random_poses(np.random.default_rng(47), 3)
        import contact_between_check as cb
        R = cb.contact_impulse_between(om, desc, q, qd, targets, bases, [0.5] * 3, poses, None, None, None, 0.0, 4)
        _COVER.update(B=B, rows=rows, idx=idx, targets=targets, bases=bases, poses=poses, R=R, desc=desc)
    return _COVER


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the solve's grid holds, plus a ragged last group: every lane loops over several groups of 64, each with
    its own Z, its own reduction of W and its own slice of the scratch.  mixed_k3's targets and bases, B distinct rows, poisoned outputs with
    guard rows, every row group checked, every entry written.  4 sweeps, normals = NULL, active = NULL, v_normal = NULL."""
    torch = torch_cuda
    C = cover_reference(torch)
    desc, B, idx, R = C["desc"], C["B"], C["idx"], C["R"]
    hm = hip_model(desc)
    q, qd, _, _ = C["rows"].device(torch, B)
    q, qd = laid_out(q, layout), laid_out(qd, layout)
    (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, 3, layout, torch.float64)
    hm.contact_impulse_between(q, qd, C["targets"], C["bases"], [0.5] * 3, C["poses"], iterations=4, layout=layout, out=(qdn, imp, res))
    torch.cuda.synchronize()
    tol = f32_aba_forward_factor(desc.n_joints) * U64 * float(R["cond_kkt"].max())
    check_cover(qdn_rows, qdn_guard, idx, R["qd_next"], tol, label=f"between qd+ layout={layout}")
    check_cover(imp_rows, imp_guard, idx, R["impulse"].reshape(len(idx), -1), tol, label=f"between impulse layout={layout}")
    check_cover(res_rows, res_guard, idx, R["residual"], tol, label=f"between residual layout={layout}")
    assert np.abs(R["impulse"]).max() > 0.1


def test_a_bad_configuration_is_nan_in_its_own_outputs_only(torch_cuda):
    """NaN in the state of one configuration and a zero normal in another: NaN in all their outputs, every neighbour bit-identical."""
    torch = torch_cuda
    name = "pairs_k4"
    _, desc, om = model_of(name)
    hm, B, nan_row, zero_row = hip_model(desc), 130, 77, 20
    I = make_inputs(name, B, seed=3)
    I["active"][[nan_row, zero_row]] = 1
    mu = mixed_mu(4)
    for dtype in (torch.float64, torch.float32):
        for layout in (AOS, SOA):
            D = device_inputs(torch, I, B, layout, dtype)
            good = [t.clone() for t in call(hm, D, I, mu, 10, layout)]
            q, nh = D["q"].clone(), D["normals"].clone()
            (q if layout == AOS else q.t())[nan_row, :] = float("nan")
            if layout == AOS:
                nh[zero_row, 2, :] = 0.0
            else:
                nh[6:9, zero_row] = 0.0
            D["q"], D["normals"] = q, nh
            got = call(hm, D, I, mu, 10, layout)
            torch.cuda.synchronize()
            keep = torch.ones(B, dtype=torch.bool, device="cuda")
            keep[[nan_row, zero_row]] = False
            for g, w in zip(got, good):
                g, w = (g.reshape(B, -1), w.reshape(B, -1)) if layout == AOS or g.dim() == 1 else (g.t(), w.t())
                assert torch.isnan(g[nan_row]).all() and torch.isnan(g[zero_row]).all(), f"layout={layout} {dtype}: a bad configuration has numbers in its outputs"
                assert not torch.isnan(w).any() and torch.equal(g[keep], w[keep]), f"layout={layout} {dtype}: a neighbour of a bad configuration changed"


def test_reserve_capture_replay_and_two_contexts(torch_cuda):
    """reserve(B) keeps the rooted size: one call grows the scratch, then the entry point captured in a graph (it allocates nothing)
    replays to the bits of the eager call; two contexts on two streams at once give the bits of the default context."""
    torch = torch_cuda
    name = "pairs_k4"
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 1000
    I = make_inputs(name, B, seed=4)
    mu = mixed_mu(4)
    D = device_inputs(torch, I, B, AOS, torch.float64)
    ref = [t.clone() for t in call(hm, D, I, mu, 25, AOS)]
    torch.cuda.synchronize()
    views, streams = [hm.context(), hm.context()], [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[torch.zeros_like(t) for t in ref] for _ in views]
    for view in views:
        view.reserve(B)
    for view, s, o in zip(views, streams, outs):  # both in flight before either is waited for
        with torch.cuda.stream(s):
            call(view, D, I, mu, 25, AOS, tuple(o))
    for view, s, o in zip(views, streams, outs):
        view.check(s.cuda_stream)
        for got, want in zip(o, ref):
            assert torch.equal(got, want)
    view, s, o = views[0], streams[0], outs[0]
    for t in o:
        t.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call(view, D, I, mu, 25, AOS, tuple(o))
    torch.cuda.synchronize()
    assert not any(t.any() for t in o)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(o, ref):
        assert torch.equal(got, want)
    for view in views:
        view.close()


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_in_place_warm_start_gives_the_bits_of_the_out_of_place_call(torch_cuda, layout):
    torch = torch_cuda
    name = "pairs_k4"
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 150
    I = make_inputs(name, B, seed=5)
    mu = mixed_mu(4)
    D = device_inputs(torch, I, B, layout, torch.float64)
    _, first, _ = call(hm, D, I, mu, 5, layout)
    start = first.clone()
    want = [t.clone() for t in call(hm, D, I, mu, 5, layout, init=start)]
    qdn, res = torch.empty_like(want[0]), torch.empty_like(want[2])
    call(hm, D, I, mu, 5, layout, (qdn, first, res), init=first)
    torch.cuda.synchronize()
    assert torch.equal(start, want[1]) is False  # five more sweeps moved the impulses
    for got, w in zip((qdn, first, res), want):
        assert torch.equal(got, w)


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    name = "pairs_k4"
    _, desc, om = model_of(name)
    hm, B, K = hip_model(desc), 10, 4
    lib = _lib.load()
    I = make_inputs(name, B)
    q, qd, nh, vn = (dev(torch, I[k]) for k in ("q", "qd", "normals", "v_normal"))
    act = dev(torch, I["active"], torch.int32)
    init = torch.zeros((B, K, 6), device="cuda", dtype=torch.float64)
    qdn, qdn_guard = poisoned(torch, B, (desc.nv,), torch.float64)
    imp, imp_guard = poisoned(torch, B, (K, 6), torch.float64)
    res, res_guard = poisoned(torch, B, (), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    tgt, base, mus = np.array(I["targets"], dtype=np.int32), np.array(I["bases"], dtype=np.int32), np.full(K, 0.5)
    ident = np.tile(kc.IDENTITY12, (K, 1))
    skewed, mirrored = ident.copy(), ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    mirrored[0, 8] = -1.0
    keep = [np.array([2, 6, 1000, 3], dtype=np.int32), np.array([-1, 2, 3, 4], dtype=np.int32), np.array([0.5, -0.1, 0.5, 0.5]),
            np.array([0.5, 0.5, np.inf, 0.5]), np.array([np.nan, 0.5, 0.5, 0.5]),
            np.array([12, 19, -1, 3], dtype=np.int32), np.array([12, 23, -2, 3], dtype=np.int32), np.array([12, 23, -1, desc.n_joints], dtype=np.int32)]

    def untouched(what):
        assert lib.mh_last_error(), what
        for t in (qdn, qdn_guard, imp, imp_guard, res, res_guard):
            assert torch.isnan(t).all(), what

    def go(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), n=K, t=tgt.ctypes.data, b=base.ctypes.data, p=None, mu=mus.ctypes.data, nh=nh.data_ptr(),
           act=act.data_ptr(), vn=vn.data_ptr(), init=init.data_ptr(), eps=0.0, it=10, out=qdn.data_ptr(), imp=imp.data_ptr(), res=res.data_ptr()):
        st = fn(hm._h, B, q, qd, n, t, b, p, mu, nh, act, vn, init, eps, it, ctypes.byref(opts), out, imp, res)
        torch.cuda.synchronize()
        return st

    refused = {"base is the target": dict(b=keep[5].ctypes.data), "base below -1": dict(b=keep[6].ctypes.data), "base out of range": dict(b=keep[7].ctypes.data),
               "NULL q": dict(q=None), "NULL qd": dict(qd=None), "NULL qd_out": dict(out=None), "NULL target_joints": dict(t=None), "NULL mu": dict(mu=None),
               "no targets": dict(n=0), "too many targets": dict(n=9), "joint out of range": dict(t=keep[0].ctypes.data),
               "the root body": dict(t=keep[1].ctypes.data), "pose not orthonormal": dict(p=skewed.ctypes.data), "pose a reflection": dict(p=mirrored.ctypes.data),
               "negative mu": dict(mu=keep[2].ctypes.data), "infinite mu": dict(mu=keep[3].ctypes.data), "NaN mu": dict(mu=keep[4].ctypes.data),
               "negative compliance": dict(eps=-1.0e-9), "NaN compliance": dict(eps=float("nan")), "no sweeps": dict(it=0), "too many sweeps": dict(it=4097),
               "qd_out is q": dict(out=q.data_ptr()), "qd_out is qd": dict(out=qd.data_ptr()), "impulse_out overlaps normals": dict(imp=nh.data_ptr()),
               "impulse_out is part of impulse_init": dict(imp=init.data_ptr() + 48, init=init.data_ptr()), "residual_out is v_normal": dict(res=vn.data_ptr()),
               "qd_out overlaps active": dict(out=act.data_ptr()), "outputs overlap": dict(imp=qdn.data_ptr() + 16),
               "residual_out inside impulse_out": dict(res=imp.data_ptr() + 8)}
    for sfx in ("f64", "f32"):
        for what, kw in refused.items():
            assert go(getattr(lib, "mh_contact_impulse_between_" + sfx), **kw) == INVALID, what
            untouched(what)
    fn = lib.mh_contact_impulse_between_f64
    before = [t.clone() for t in (q, qd, nh, vn, act, init)]
    assert go(fn, B=0) == 0 and go(fn, B=0, q=None, qd=None, out=None, imp=None, res=None) == 0
    untouched("B = 0")
    locked = hip_model(desc)
    modes = np.zeros(desc.n_joints, dtype=np.int32)
    modes[3] = 1
    locked.set_joint_source_modes(modes)
    assert fn(locked._h, B, q.data_ptr(), qd.data_ptr(), K, tgt.ctypes.data, base.ctypes.data, None, mus.ctypes.data, None, None, None, None, 0.0, 10,
              ctypes.byref(opts), qdn.data_ptr(), imp.data_ptr(), res.data_ptr()) == INVALID
    untouched("acceleration-source joints")
    assert go(fn, p=ident.ctypes.data, imp=None, res=None) == 0  # the optional outputs absent
    assert not torch.isnan(qdn).any() and torch.isnan(imp).all() and torch.isnan(res).all()
    assert go(fn, nh=None, act=None, vn=None, init=None) == 0
    for t, gd in ((qdn, qdn_guard), (imp, imp_guard), (res, res_guard)):
        assert not torch.isnan(t).any() and torch.isnan(gd).all()
    assert go(fn, init=imp.data_ptr()) == 0  # the one permitted overlap: impulse_out == impulse_init exactly
    assert all(torch.equal(x, y) for x, y in zip((q, qd, nh, vn, act, init), before))
    with pytest.raises(_lib.MecanoHipError):
        hm.contact_impulse_between(q, qd, I["targets"], I["bases"][:2], mus)  # two bases for four targets
    with pytest.raises(_lib.MecanoHipError):
        hm.contact_impulse_between(q, qd, I["targets"], I["bases"], [0.5])
