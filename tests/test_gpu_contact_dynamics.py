"""mh_contact_impulse_* on the device against the CPU checker running the same sweeps (tests/contact_dynamics_check.py, pinned by
tests/test_contact_dynamics_cpu.py), through the C-ABI (HipModel.contact_impulse is the ctypes call).  Every output is poisoned and has a
guard row behind it: entries left unwritten and writes past the end show.

Parity bound: helpers.close_aba on (qd_next, impulse) with cond_inf of the KKT matrix of the stick system (all contacts as point
constraints with the call's compliance) -- the sweeps are nonexpansive, so what the device can differ by is what rounding does to S, b and
the propagation, and those are the solves that matrix conditions.  u = 2^-53 or 2^-24; fp32 is held against the fp64 checker on the
fp32-rounded inputs.  Beside it the momentum balance H (qd_out - qd) = J^T impulse through the checker's H and J with cond_inf(H), exact
zeros in the rows that take no part, and residual_out to the same bound.  The converged tests read the physics instead: the natural
residual of the device's impulses through the checker's S and b."""
import ctypes

import numpy as np
import pytest

import contact_dynamics_check as cd
import helpers as hp
import kinematics_check as kc
from helpers import DistinctRows, U32, check_cover, close_aba, f32_aba_forward_factor, group_cover, poisoned
from test_contact_dynamics_cpu import CASES, make_inputs, model_of
from test_gpu_constrained_dynamics import (AOS, B_MAX, BATCHES, INVALID, SOA, U64, dev, hip_model, hold_residual, laid_out, moved_inputs, outputs,
                                           scattered_description, torch_cuda)  # noqa: F401

pytestmark = pytest.mark.gpu

SWEEPS = {"arm7": 50, "humanoid30": 50, "humanoid30_k8": 20}  # k8: the streamed fp64 path; no convergence is claimed there
_REFS = {}


def reference(name, dtype_name, mu):
    """(inputs, checker result) of B_MAX configurations with random active and v_normal, once per (case, precision, mu)"""
    key = (name, dtype_name, mu)
    if key not in _REFS:
        I = make_inputs(name, B_MAX, seed=1, dtype=np.float64 if dtype_name == "f64" else np.float32)
        _, desc, om = model_of(name)
        K = len(I["targets"])
        _REFS[key] = (I, cd.contact_impulse(om, desc, I["q"], I["qd"], I["targets"], [mu] * K, I["poses"], I["normals"], I["active"], I["v_normal"],
                                            I["compliance"], SWEEPS[name]))
    return _REFS[key]


def device_inputs(torch, I, B, layout, dtype):
    d = {k: laid_out(dev(torch, I[k][:B], dtype), layout) for k in ("q", "qd", "normals", "v_normal")}
    d["active"] = laid_out(dev(torch, I["active"][:B], torch.int32), layout)
    return d


def three_outputs(torch, B, nv, K, layout, dtype):
    qdn = outputs(torch, B, (nv,), layout, dtype)
    imp = outputs(torch, B, (K, 6), layout, dtype)
    res, res_guard = poisoned(torch, B, (), dtype)
    return qdn, imp, (res.view(B), res.view(B), res_guard)


def call(hm, D, I, mu, sweeps, layout, out=None, init=None, active=True, v_normal=True):
    K = len(I["targets"])
    return hm.contact_impulse(D["q"], D["qd"], I["targets"], [mu] * K, I["poses"], D["normals"], D["active"] if active else None,
                              D["v_normal"] if v_normal else None, I["compliance"], sweeps, init, layout, out)


@pytest.mark.parametrize("mu", [0.0, 0.5])
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name", list(CASES))
def test_matches_checker(torch_cuda, name, layout, dtype_name, mu):
    torch = torch_cuda
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R = reference(name, dtype_name, mu)
    _, desc, om = model_of(name)
    hm = hip_model(desc)
    K, n = len(I["targets"]), desc.n_joints
    for B in BATCHES:
        label = f"{name} B={B} layout={layout} {dtype_name} mu={mu}"
        D = device_inputs(torch, I, B, layout, dtype)
        (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, K, layout, dtype)
        call(hm, D, I, mu, SWEEPS[name], layout, (qdn, imp, res))
        torch.cuda.synchronize()
        assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
        v, p = qdn_rows.cpu().numpy().astype(np.float64), imp_rows.cpu().numpy().astype(np.float64).reshape(B, K, 6)
        r = res_rows.cpu().numpy().astype(np.float64)
        assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
        assert not p[:, :, :3].any(), label + ": an angular row is not exactly zero"
        assert not p[I["active"][:B] == 0].any(), label + ": an open contact has an impulse"
        print(f"{label}: |qd+ - ref| = {np.abs(v - R['qd_next'][:B]).max():.3e}, |impulse - ref| = {np.abs(p - R['impulse'][:B]).max():.3e}, "
              f"|residual - ref| = {np.abs(r - R['residual'][:B]).max():.3e}, cond_kkt <= {R['cond_kkt'][:B].max():.2e}")
        close_aba(np.concatenate([v, p.reshape(B, -1)], axis=1), np.concatenate([R["qd_next"][:B], R["impulse"][:B].reshape(B, -1)], axis=1), None, n,
                  u, label=label + " (qd+, impulse)", conds=R["cond_kkt"][:B])
        close_aba(r[:, None], R["residual"][:B, None], None, n, u, label=label + " residual", conds=R["cond_kkt"][:B])
        H, JTp = R["H"][:B], np.einsum("bji,bj->bi", R["J"][:B], p.reshape(B, -1))
        Hv, Hq = np.einsum("bij,bj->bi", H, v), np.einsum("bij,bj->bi", H, I["qd"][:B])
        scale = np.abs(Hv).max(axis=1) + np.abs(Hq).max(axis=1) + np.abs(JTp).max(axis=1)
        hold_residual(np.abs(Hv - Hq - JTp).max(axis=1), scale, R["cond_H"][:B], n, u, label + " momentum balance")


@pytest.mark.parametrize("mu", [0.0, 0.5, 100.0])
@pytest.mark.parametrize("name", ["arm7", "humanoid30"])
def test_converged_impulses_solve_the_contact_problem(torch_cuda, name, mu):
    """1000 sweeps in fp64, every contact closed: the device's impulses are the minimiser -- their natural residual through the checker's S
    and b vanishes -- lie in their cones, and at mu = 0 are the enumerated complementarity solution."""
    torch = torch_cuda
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 64
    I = make_inputs(name, B)
    K = len(I["targets"])
    D = device_inputs(torch, I, B, AOS, torch.float64)
    _, imp, res = call(hm, D, I, mu, 1000, AOS, active=False, v_normal=False)
    torch.cuda.synchronize()
    lam = imp.cpu().numpy()[:, :, 3:]
    T = cd.terms(om, desc, I["q"], I["qd"], I["targets"], I["poses"], I["normals"])
    scale = max(1.0, np.abs(lam).max())
    nat = cd.natural_residual(T["S"], T["b"], T["n"], [mu] * K, None, I["compliance"], lam).max()
    print(f"{name} mu={mu}: natural residual {nat:.2e}, |lam| <= {scale:.2f}, residual_out <= {float(res.max()):.2e}")
    assert nat <= 1.0e-9 * scale
    ln = np.einsum("bki,bki->bk", T["n"], lam)
    lt = np.linalg.norm(lam - ln[:, :, None] * T["n"], axis=2)
    assert ln.min() >= -1.0e-12 * scale and (lt <= mu * ln + 1.0e-12 * scale).all() and np.abs(lam).max() > 0.1
    if mu == 0.0:
        want = cd.frictionless_exact(T["S"], T["b"], T["n"], None, I["compliance"])
        assert np.abs(lam - want).max() <= 1.0e-9 * scale


def set_path(hm, path):
    from mecano_amd import _lib
    _lib.check(_lib.load().mh_internal_contact_path(hm._h, path))


@pytest.mark.parametrize("name,dtype_name", [("humanoid30", "f64"), ("humanoid30_k8", "f32"), ("arm7", "f32")])
def test_resident_and_streamed_solves_give_the_same_bits(torch_cuda, name, dtype_name):
    """S in LDS against S streamed from scratch, each forced (K = 4 in fp64, K = 8 and K = 1 in fp32 take LDS on their own)."""
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 200
    I = make_inputs(name, B, seed=2, dtype=np.float64 if dtype_name == "f64" else np.float32)
    for layout in (AOS, SOA):
        D = device_inputs(torch, I, B, layout, dtype)
        got = []
        for path in (1, 0, -1):
            set_path(hm, path)
            got.append([t.clone() for t in call(hm, D, I, 0.5, 30, layout)])
        torch.cuda.synchronize()
        assert got[0][1].any()
        for a, b, c in zip(*got):
            assert torch.equal(a, b) and torch.equal(a, c), f"{name} {dtype_name} layout={layout}: the two paths differ"
    set_path(hm, -1)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("holes,relist", [(0, False), (0, True), (2, False)])
def test_scattered_index_maps(torch_cuda, holes, relist, layout, dtype_name):
    """The humanoid of test_matches_checker on maps that send every DoF and every configuration entry somewhere else (also with two indices
    of each space owned by no joint, holding 7.0 in q and qd, and with its joints re-listed and the targets translated), mu = 0.5, with
    that test's targets, poses, normals, active and v_normal, against ITS reference -- the checker on the identity description -- under its
    bound: close_aba on (qd+, impulse) and on the residual with cond_inf(KKT).  Both forms of the solve, S resident in LDS and S streamed,
    each forced.  q and qd go in through the maps, qd+ comes back through the DoF map; impulses and residuals do not move.  Guard rows
    stay poisoned; read without moving it back qd+ misses the reference by more than 1e-3."""
    torch = torch_cuda
    name, mu = "humanoid30", 0.5
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R = reference(name, dtype_name, mu)
    _, desc, om = model_of(name)
    d, pv, pq, targets, _, order = scattered_description(name, desc, holes, relist, I["targets"])
    hm = hip_model(d)
    assert relist or hm.kernel_variant.startswith("topo:"), hm.kernel_variant
    B, K, n, nv = 70, len(targets), desc.n_joints, d.nv
    D = moved_inputs(torch, I, B, pv, pq, d, order, layout, dtype, keys=("q", "qd", "normals", "v_normal"))
    J = dict(I, targets=targets)
    try:
        for path in (1, 0):
            label = f"scattered holes={holes} relist={relist} path={path} layout={layout} {dtype_name}"
            set_path(hm, path)
            (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, nv, K, layout, dtype)
            call(hm, D, J, mu, SWEEPS[name], layout, (qdn, imp, res))
            torch.cuda.synchronize()
            assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
            raw, p = qdn_rows.cpu().numpy().astype(np.float64), imp_rows.cpu().numpy().astype(np.float64).reshape(B, K, 6)
            v, r = hp.from_v(raw, pv)[0], res_rows.cpu().numpy().astype(np.float64)
            assert np.all(hp.from_v(raw, pv)[1] == hp.UNOWNED), label + ": entries of qd_out no joint owns do not hold those of qd"
            assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
            assert not p[:, :, :3].any() and not p[I["active"][:B] == 0].any(), label
            close_aba(np.concatenate([v, p.reshape(B, -1)], axis=1), np.concatenate([R["qd_next"][:B], R["impulse"][:B].reshape(B, -1)], axis=1), None,
                      n, u, label=label + " (qd+, impulse)", conds=R["cond_kkt"][:B])
            close_aba(r[:, None], R["residual"][:B, None], None, n, u, label=label + " residual", conds=R["cond_kkt"][:B])
            hp.assert_misses(hp.keep_order(raw, pv), R["qd_next"][:B], label + " qd+")
    finally:
        set_path(hm, -1)


def test_a_bad_configuration_is_nan_in_its_own_outputs_only(torch_cuda):
    """NaN in the state of one configuration (trace S_kk is no positive number) and a zero normal in another: NaN in all their outputs,
    every neighbour bit-identical."""
    torch = torch_cuda
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B, nan_row, zero_row = hip_model(desc), 130, 77, 20
    I = make_inputs(name, B, seed=3)
    I["active"][[nan_row, zero_row]] = 1
    for dtype in (torch.float64, torch.float32):
        for layout in (AOS, SOA):
            D = device_inputs(torch, I, B, layout, dtype)
            good = [t.clone() for t in call(hm, D, I, 0.5, 10, layout)]
            q, nh = D["q"].clone(), D["normals"].clone()
            (q if layout == AOS else q.t())[nan_row, :] = float("nan")
            if layout == AOS:
                nh[zero_row, 2, :] = 0.0
            else:
                nh[6:9, zero_row] = 0.0
            D["q"], D["normals"] = q, nh
            got = call(hm, D, I, 0.5, 10, layout)
            torch.cuda.synchronize()
            keep = torch.ones(B, dtype=torch.bool, device="cuda")
            keep[[nan_row, zero_row]] = False
            for g, w in zip(got, good):
                g, w = (g.reshape(B, -1), w.reshape(B, -1)) if layout == AOS or g.dim() == 1 else (g.t(), w.t())
                assert torch.isnan(g[nan_row]).all() and torch.isnan(g[zero_row]).all(), f"layout={layout} {dtype}: a bad configuration has numbers in its outputs"
                assert not torch.isnan(w).any() and torch.equal(g[keep], w[keep]), f"layout={layout} {dtype}: a neighbour of a bad configuration changed"


_COVER = {}


def cover_reference(torch):
    if not _COVER:
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        sys_, desc, om = model_of("humanoid30")
        B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
        rows = DistinctRows(sys_, 256, seed=41)
        idx = group_cover(B, grid)
        q, qd, _, _ = rows.rows(idx)
        targets, poses = [6, 12], kc.random_poses(np.random.default_rng(45), 2)
        R = cd.contact_impulse(om, desc, q, qd, targets, [0.5, 0.5], poses, None, None, None, 0.0, 4)
        _COVER.update(B=B, rows=rows, idx=idx, targets=targets, poses=poses, R=R, desc=desc)
    return _COVER


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the solve's grid holds (8 per CU at K = 2), plus a ragged last group: every lane loops over several groups
    of 64.  B distinct rows, poisoned outputs with guard rows, every row group checked, every entry written.  Both feet, 4 sweeps,
    normals = NULL (the root's z axis), active = NULL, v_normal = NULL."""
    torch = torch_cuda
    C = cover_reference(torch)
    desc, B, idx, R = C["desc"], C["B"], C["idx"], C["R"]
    hm = hip_model(desc)
    q, qd, _, _ = C["rows"].device(torch, B)
    q, qd = laid_out(q, layout), laid_out(qd, layout)
    (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, 2, layout, torch.float64)
    hm.contact_impulse(q, qd, C["targets"], [0.5, 0.5], C["poses"], iterations=4, layout=layout, out=(qdn, imp, res))
    torch.cuda.synchronize()
    tol = f32_aba_forward_factor(desc.n_joints) * U64 * float(R["cond_kkt"].max())
    check_cover(qdn_rows, qdn_guard, idx, R["qd_next"], tol, label=f"qd+ layout={layout}")
    check_cover(imp_rows, imp_guard, idx, R["impulse"].reshape(len(idx), -1), tol, label=f"impulse layout={layout}")
    check_cover(res_rows, res_guard, idx, R["residual"], tol, label=f"residual layout={layout}")
    assert np.abs(R["impulse"]).max() > 0.1


def test_reserve_capture_replay_and_two_contexts(torch_cuda):
    """reserve(B), one call, then the entry point captured in a graph (it allocates nothing) replays to the bits of the eager call; two
    contexts on two streams at once give the bits of the default context."""
    torch = torch_cuda
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 1000
    I = make_inputs(name, B, seed=4)
    D = device_inputs(torch, I, B, AOS, torch.float64)
    ref = [t.clone() for t in call(hm, D, I, 0.5, 25, AOS)]
    torch.cuda.synchronize()
    views, streams = [hm.context(), hm.context()], [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[torch.zeros_like(t) for t in ref] for _ in views]
    for view in views:
        view.reserve(B)
    for view, s, o in zip(views, streams, outs):  # both in flight before either is waited for
        with torch.cuda.stream(s):
            call(view, D, I, 0.5, 25, AOS, tuple(o))
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
            call(view, D, I, 0.5, 25, AOS, tuple(o))
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
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 150
    I = make_inputs(name, B, seed=5)
    D = device_inputs(torch, I, B, layout, torch.float64)
    _, first, _ = call(hm, D, I, 0.5, 5, layout)
    start = first.clone()
    want = [t.clone() for t in call(hm, D, I, 0.5, 5, layout, init=start)]
    qdn, res = torch.empty_like(want[0]), torch.empty_like(want[2])
    call(hm, D, I, 0.5, 5, layout, (qdn, first, res), init=first)
    torch.cuda.synchronize()
    assert torch.equal(start, want[1]) is False  # five more sweeps moved the impulses
    for got, w in zip((qdn, first, res), want):
        assert torch.equal(got, w)


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    name = "humanoid30"
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
    tgt, mus = np.array(I["targets"], dtype=np.int32), np.full(K, 0.5)
    ident = np.tile(kc.IDENTITY12, (K, 1))
    skewed, mirrored = ident.copy(), ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    mirrored[0, 8] = -1.0
    keep = [np.array([2, 6, 1000, 3], dtype=np.int32), np.array([-1, 2, 3, 4], dtype=np.int32), np.array([0.5, -0.1, 0.5, 0.5]),
            np.array([0.5, 0.5, np.inf, 0.5]), np.array([np.nan, 0.5, 0.5, 0.5])]

    def untouched(what):
        assert lib.mh_last_error(), what
        for t in (qdn, qdn_guard, imp, imp_guard, res, res_guard):
            assert torch.isnan(t).all(), what

    def go(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), n=K, t=tgt.ctypes.data, p=None, mu=mus.ctypes.data, nh=nh.data_ptr(), act=act.data_ptr(),
           vn=vn.data_ptr(), init=init.data_ptr(), eps=0.0, it=10, out=qdn.data_ptr(), imp=imp.data_ptr(), res=res.data_ptr()):
        st = fn(hm._h, B, q, qd, n, t, p, mu, nh, act, vn, init, eps, it, ctypes.byref(opts), out, imp, res)
        torch.cuda.synchronize()
        return st

    refused = {"NULL q": dict(q=None), "NULL qd": dict(qd=None), "NULL qd_out": dict(out=None), "NULL target_joints": dict(t=None), "NULL mu": dict(mu=None),
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
            assert go(getattr(lib, "mh_contact_impulse_" + sfx), **kw) == INVALID, what
            untouched(what)
    before = [t.clone() for t in (q, qd, nh, vn, act, init)]
    assert go(lib.mh_contact_impulse_f64, B=0) == 0 and go(lib.mh_contact_impulse_f64, B=0, q=None, qd=None, out=None, imp=None, res=None) == 0
    untouched("B = 0")
    locked = hip_model(desc)
    modes = np.zeros(desc.n_joints, dtype=np.int32)
    modes[3] = 1
    locked.set_joint_source_modes(modes)
    assert lib.mh_contact_impulse_f64(locked._h, B, q.data_ptr(), qd.data_ptr(), K, tgt.ctypes.data, None, mus.ctypes.data, None, None, None, None, 0.0, 10,
                                      ctypes.byref(opts), qdn.data_ptr(), imp.data_ptr(), res.data_ptr()) == INVALID
    untouched("acceleration-source joints")
    assert go(lib.mh_contact_impulse_f64, p=ident.ctypes.data, it=4096, imp=None, res=None) == 0  # the most sweeps, the optional outputs absent
    assert not torch.isnan(qdn).any() and torch.isnan(imp).all() and torch.isnan(res).all()
    assert go(lib.mh_contact_impulse_f64, nh=None, act=None, vn=None, init=None) == 0
    for t, gd in ((qdn, qdn_guard), (imp, imp_guard), (res, res_guard)):
        assert not torch.isnan(t).any() and torch.isnan(gd).all()
    assert all(torch.equal(x, y) for x, y in zip((q, qd, nh, vn, act, init), before))
    with pytest.raises(_lib.MecanoHipError):
        hm.contact_impulse(q, qd, I["targets"], [0.5])  # one coefficient for four targets
    with pytest.raises(_lib.MecanoHipError):
        hm.contact_impulse(q, qd, I["targets"], mus, normals=nh[:, :2].contiguous())
    with pytest.raises(ValueError):
        hm.contact_impulse(q, qd, I["targets"], mus, active=act.to(torch.int64))
