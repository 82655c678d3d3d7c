"""mh_joint_limit_impulse_* on the device against the CPU checker running the same sweeps (tests/joint_limits_check.py, pinned by
tests/test_joint_limits_cpu.py), through the C-ABI (HipModel.joint_limit_impulse is the ctypes call).  Every output is poisoned and has a
guard row behind it: entries left unwritten and writes past the end show.

Parity bound: helpers.close_aba on (qd_next, impulse) and on the residual with cond_inf of the stick system, the KKT matrix
[[H, E_c^T], [E_c, -eps I]] over the closed rows -- the sweeps are nonexpansive, so what the device can differ by is what rounding does to
S, b and the combination of the columns, and those are the solves that matrix conditions: 8 sqrt(8 n) cond u.  u = 2^-53 or 2^-24; fp32 is
held against the fp64 checker on the fp32-rounded inputs (limits +-1, margin 0.25, erp 50 are exact in fp32; no q of a listed joint is
within 1e-3 of a closing threshold).  A numpy fp32 run of these sweeps stays at <= 0.06 of that bound; what the device achieves is in
profiles/joint_limits_parity_errors.json.  Beside it: exact zeros on open rows and the momentum balance H (qd_out - qd) = E^T impulse
through the checker's H with cond_inf(H).  The converged tests read the physics instead: the natural residual of the device's impulses
through the checker's S and b."""
import ctypes

import numpy as np
import pytest

import helpers as hp
import joint_limits_check as jl
from helpers import DistinctRows, U32, check_cover, close_aba, f32_aba_forward_factor, group_cover, poisoned
from test_gpu_constrained_dynamics import (AOS, B_MAX, BATCHES, INVALID, SOA, U64, dev, hip_model, hold_residual, laid_out, outputs,
                                           scattered_description, torch_cuda)  # noqa: F401
from test_joint_limits_cpu import ERP, LOWER, MARGIN, UPPER, make_inputs, model_of

pytestmark = pytest.mark.gpu

_REFS = {}


def humanoid_joints(L):
    _, desc, _ = model_of("humanoid30")
    return jl.one_dof_joints(desc)[:L]


# case -> (model, listed joints: None = every 1-DoF joint)
CASES = {"arm7": ("arm7", None), "humanoid30": ("humanoid30", None), "arm7_l1": ("arm7", [4]), "humanoid30_l22": ("humanoid30", 22), "humanoid30_l23": ("humanoid30", 23)}


def case_inputs(case, B, seed=0, dtype=np.float64):
    name, joints = CASES[case]
    return name, make_inputs(name, B, seed, dtype, humanoid_joints(joints) if isinstance(joints, int) else joints)


def check(name, I, sweeps, compliance, init=None):
    _, desc, om = model_of(name)
    return jl.joint_limit_impulse(om, desc, I["q"], I["qd"], I["joints"], I["lower"], I["upper"], I["margin"], I["erp"], compliance, sweeps, init)


def reference(case, dtype_name, compliance, sweeps):
    """(model name, inputs, checker result) of B_MAX configurations, once per (case, precision, compliance, sweeps)"""
    key = (case, dtype_name, compliance, sweeps)
    if key not in _REFS:
        name, I = case_inputs(case, B_MAX, seed=1, dtype=np.float64 if dtype_name == "f64" else np.float32)
        _REFS[key] = (name, I, check(name, I, sweeps, compliance))
    return _REFS[key]


def three_outputs(torch, B, nv, L, layout, dtype):
    qdn = outputs(torch, B, (nv,), layout, dtype)
    imp = outputs(torch, B, (L,), layout, dtype)
    res, res_guard = poisoned(torch, B, (), dtype)
    return qdn, imp, (res.view(B), res.view(B), res_guard)


def device_state(torch, I, B, layout, dtype):
    return laid_out(dev(torch, I["q"][:B], dtype), layout), laid_out(dev(torch, I["qd"][:B], dtype), layout)


def call(hm, q, qd, I, sweeps, layout, out=None, init=None, compliance=0.0):
    return hm.joint_limit_impulse(q, qd, I["joints"], I["lower"], I["upper"], I["margin"], I["erp"], compliance, sweeps, init, layout, out)


def hold_parity(torch, hm, name, I, R, B, layout, dtype_name, sweeps, compliance, label, init=None, in_place=False):
    """init: the start R was computed from, [B, L]; in_place: impulse_out is impulse_init.  Returns the [B, ...] views of the three outputs."""
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    _, desc, om = model_of(name)
    L, n = len(I["joints"]), desc.n_joints
    q, qd = device_state(torch, I, B, layout, dtype)
    (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, L, layout, dtype)
    start = None if init is None else laid_out(dev(torch, init[:B], dtype), layout)
    if in_place:
        imp.copy_(start)
        start = imp
    call(hm, q, qd, I, sweeps, layout, (qdn, imp, res), init=start, compliance=compliance)
    torch.cuda.synchronize()
    assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
    v, p, r = (t.cpu().numpy().astype(np.float64) for t in (qdn_rows, imp_rows, res_rows))
    assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
    assert not p[~R["closed"][:B]].any(), label + ": an open row has an impulse"
    assert (R["s"][:B] * p >= 0).all(), label + ": a limit pulled"
    print(f"{label}: |qd+ - ref| = {np.abs(v - R['qd_next'][:B]).max():.3e}, |impulse - ref| = {np.abs(p - R['impulse'][:B]).max():.3e}, "
          f"|residual - ref| = {np.abs(r - R['residual'][:B]).max():.3e}, cond_kkt <= {R['cond_kkt'][:B].max():.2e}")
    close_aba(np.concatenate([v, p], axis=1), np.concatenate([R["qd_next"][:B], R["impulse"][:B]], axis=1), None, n, u, label=label + " (qd+, impulse)",
              conds=R["cond_kkt"][:B])
    close_aba(r[:, None], R["residual"][:B, None], None, n, u, label=label + " residual", conds=R["cond_kkt"][:B])
    H = R["H"][:B]
    ETp = np.zeros_like(v)
    ETp[:, R["d"]] = p
    Hv, Hq = np.einsum("bij,bj->bi", H, v), np.einsum("bij,bj->bi", H, I["qd"][:B])
    scale = np.abs(Hv).max(axis=1) + np.abs(Hq).max(axis=1) + np.abs(ETp).max(axis=1)
    hold_residual(np.abs(Hv - Hq - ETp).max(axis=1), scale, R["cond_H"][:B], n, u, label + " momentum balance")
    return qdn_rows, imp_rows, res_rows


@pytest.mark.parametrize("compliance", [0.0, 1.0e-6])
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_matches_checker(torch_cuda, case, layout, dtype_name, compliance):
    """arm7 (L = 7) and the humanoid's 24 one-DoF joints (streamed in fp64, resident in fp32), 50 sweeps, every batch size"""
    name, I, R = reference(case, dtype_name, compliance, 50)
    hm = hip_model(model_of(name)[1])
    for B in BATCHES:
        hold_parity(torch_cuda, hm, name, I, R, B, layout, dtype_name, 50, compliance, f"{case} B={B} layout={layout} {dtype_name} eps={compliance}")


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("case,sweeps", [("arm7", 1), ("arm7", 3), ("humanoid30", 1), ("humanoid30", 3), ("arm7_l1", 50), ("humanoid30_l22", 50),
                                         ("humanoid30_l23", 50)])
def test_few_sweeps_and_the_list_lengths_around_the_lds_boundary(torch_cuda, case, sweeps, dtype_name):
    """1 and 3 sweeps (nothing has converged: the order of the updates shows); L = 1; L = 22 / 23, the last resident and the first
    streamed length in fp64"""
    name, I, R = reference(case, dtype_name, 0.0, sweeps)
    hm = hip_model(model_of(name)[1])
    for layout in (AOS, SOA):
        hold_parity(torch_cuda, hm, name, I, R, 65, layout, dtype_name, sweeps, 0.0, f"{case} sweeps={sweeps} layout={layout} {dtype_name}")


@pytest.mark.parametrize("name", ["arm7", "humanoid30"])
def test_converged_impulses_solve_the_complementarity_problem(torch_cuda, name):
    """1000 sweeps in fp64: the natural residual of the device's impulses through the checker's S and b vanishes, no limit pulls, and
    on arm7 they are the enumerated solution."""
    torch = torch_cuda
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 64
    I = make_inputs(name, B)
    q, qd = device_state(torch, I, B, AOS, torch.float64)
    _, imp, res = call(hm, q, qd, I, 1000, AOS)
    torch.cuda.synchronize()
    T = jl.terms(om, desc, I["q"], I["qd"], I["joints"], I["lower"], I["upper"], I["margin"], I["erp"])
    lam = T["s"] * imp.cpu().numpy()
    scale = max(1.0, np.abs(lam).max())
    nat = jl.natural_residual(T["S"], T["b"], T["closed"], 0.0, lam).max()
    print(f"{name}: natural residual {nat:.2e}, |lam| <= {scale:.2f}, residual_out <= {float(res.max()):.2e}")
    assert nat <= 1.0e-9 * scale
    assert lam.min() >= -1.0e-12 * scale and np.abs(lam).max() > 0.1
    if name == "arm7":
        assert np.abs(lam - jl.exact(T["S"], T["b"], T["closed"], 0.0)).max() <= 1.0e-9 * scale


def set_path(hm, path):
    from mecano_amd import _lib
    _lib.check(_lib.load().mh_internal_limit_path(hm._h, path))


def _scattered_reference(dtype_name, sweeps):
    """The humanoid's first 22 one-DoF joints listed in DESCENDING order (what fp64 can still hold in LDS), 70 configurations: inputs in the
    identity description's index space and the checker's result on them, once per precision and sweep count, never modified."""
    key = ("scattered", dtype_name, sweeps)
    if key not in _REFS:
        I = make_inputs("humanoid30", 70, 1, np.float64 if dtype_name == "f64" else np.float32, humanoid_joints(22)[::-1])
        _REFS[key] = (I, check("humanoid30", I, sweeps, 0.0))
    return _REFS[key]


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("holes,relist", [(0, False), (0, True), (2, False)])
def test_scattered_index_maps(torch_cuda, holes, relist, layout, dtype_name):
    """The humanoid on maps that send every DoF and every configuration entry somewhere else -- so that a listed joint's configuration
    index is not its DoF index, which the host resolves one by one before it indexes columns of H^-1 with them -- (also with two indices of
    each space owned by no joint, holding 7.0 in q and qd, and with the joints re-listed and the list translated), 22 joints listed in
    descending order, 3 sweeps (nothing has converged: the order of the updates shows), against the checker on the IDENTITY description
    under hold_parity's bound: close_aba on (qd+, impulse) and on the residual with cond_inf(KKT).  The resident and the streamed form,
    each forced.  q and qd go in through the maps, qd+ comes back through the DoF map; impulses (one per listed joint, in list order) and
    residuals do not move.  Guard rows stay poisoned; read without moving it back qd+ misses the reference by more than 1e-3."""
    torch = torch_cuda
    name, sweeps, B = "humanoid30", 3, 70
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R = _scattered_reference(dtype_name, sweeps)
    _, desc, om = model_of(name)
    assert not R["bad"].any() and R["closed"].any() and np.abs(R["impulse"]).max() > 0.1
    d, pv, pq, joints, _, _ = scattered_description(name, desc, holes, relist, I["joints"])
    d_idx, c_idx = jl.joint_indices(desc, I["joints"])
    assert np.any(pv[d_idx] != pq[c_idx]), "every listed joint's configuration index is its DoF index"
    hm = hip_model(d)
    assert relist or hm.kernel_variant.startswith("topo:"), hm.kernel_variant
    L, n, nv = len(joints), desc.n_joints, d.nv
    q = laid_out(dev(torch, hp.to_q(I["q"], pq, d.nq), dtype), layout)
    qd = laid_out(dev(torch, hp.to_v(I["qd"], pv, nv), dtype), layout)
    J = dict(I, joints=joints)
    try:
        for path in (1, 0):
            label = f"scattered holes={holes} relist={relist} path={path} layout={layout} {dtype_name}"
            set_path(hm, path)
            (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, nv, L, layout, dtype)
            call(hm, q, qd, J, sweeps, layout, (qdn, imp, res))
            torch.cuda.synchronize()
            assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
            raw, p, r = (t.cpu().numpy().astype(np.float64) for t in (qdn_rows, imp_rows, res_rows))
            v = hp.from_v(raw, pv)[0]
            assert np.all(hp.from_v(raw, pv)[1] == hp.UNOWNED), label + ": entries of qd_out no joint owns do not hold those of qd"
            assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
            assert not p[~R["closed"]].any() and (R["s"] * p >= 0).all(), label
            close_aba(np.concatenate([v, p], axis=1), np.concatenate([R["qd_next"], R["impulse"]], axis=1), None, n, u, label=label + " (qd+, impulse)",
                      conds=R["cond_kkt"])
            close_aba(r[:, None], R["residual"][:, None], None, n, u, label=label + " residual", conds=R["cond_kkt"])
            hp.assert_misses(hp.keep_order(raw, pv), R["qd_next"], label + " qd+")
    finally:
        set_path(hm, -1)


@pytest.mark.parametrize("case,dtype_name", [("humanoid30_l22", "f64"), ("humanoid30", "f32"), ("arm7", "f32")])
def test_resident_and_streamed_solves_give_the_same_bits(torch_cuda, case, dtype_name):
    """S in LDS against S streamed from the columns, each forced"""
    torch = torch_cuda
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    name, I = case_inputs(case, 200, seed=2, dtype=np.float64 if dtype_name == "f64" else np.float32)
    hm = hip_model(model_of(name)[1])
    for layout in (AOS, SOA):
        q, qd = device_state(torch, I, 200, layout, dtype)
        got = []
        for path in (1, 0, -1):
            set_path(hm, path)
            got.append([t.clone() for t in call(hm, q, qd, I, 30, layout, compliance=1.0e-6)])
        torch.cuda.synchronize()
        assert got[0][1].any()
        for a, b, c in zip(*got):
            assert torch.equal(a, b) and torch.equal(a, c), f"{case} {dtype_name} layout={layout}: the two paths differ"
    set_path(hm, -1)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_sixty_four_rows_on_the_wide_tree(torch_cuda, dtype_name):
    """tree128 with its first 64 one-DoF joints, B = 65: the cap, streaming at either precision, scratch beyond what reserve set aside.
    In fp32 this is a check of cover and NaN, not of numbers: cond_kkt is 1e7 here, so the bound 8 sqrt(8 n) cond_kkt 2^-24 is of order 1e2
    relative on every row.  The fp32 check of long lists with a bound that bites is test_gpu_joint_limits_wide.py::
    test_the_fp32_lds_boundary_and_the_cap_on_the_comb (comb16x4: the bound is 1e-2)."""
    torch = torch_cuda
    name = "tree128"
    _, desc, om = model_of(name)
    joints = jl.one_dof_joints(desc)[:64]
    assert len(joints) == 64
    key = ("tree128", dtype_name)
    if key not in _REFS:
        I = make_inputs(name, 65, seed=6, dtype=np.float64 if dtype_name == "f64" else np.float32, joints=joints)
        _REFS[key] = (I, check(name, I, 20, 0.0))
    I, R = _REFS[key]
    hm = hip_model(desc)
    hm.reserve(65)
    for layout in (AOS, SOA):
        hold_parity(torch, hm, name, I, R, 65, layout, dtype_name, 20, 0.0, f"tree128 L=64 layout={layout} {dtype_name}")


def test_a_bad_configuration_is_nan_in_its_own_outputs_only(torch_cuda):
    """NaN in q of a listed joint, in qd of a closed row and in impulse_init of a closed row, one configuration each: NaN in all their
    outputs, every neighbour bit-identical."""
    torch = torch_cuda
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B, bad_rows = hip_model(desc), 130, [20, 77, 101]
    I = make_inputs(name, B, seed=3)
    T = jl.terms(om, desc, I["q"], I["qd"], I["joints"], I["lower"], I["upper"], I["margin"], I["erp"])
    first_closed = [int(np.nonzero(T["closed"][r])[0][0]) for r in bad_rows]
    L = len(I["joints"])
    for dtype in (torch.float64, torch.float32):
        for layout in (AOS, SOA):
            q, qd = device_state(torch, I, B, layout, dtype)
            init = laid_out(torch.full((B, L), 0.25, device="cuda", dtype=dtype), layout)
            good = [t.clone() for t in call(hm, q, qd, I, 10, layout, init=init)]
            q, qd, init = q.clone(), qd.clone(), init.clone()
            (q if layout == AOS else q.t())[bad_rows[0], int(T["c"][3])] = float("nan")
            (qd if layout == AOS else qd.t())[bad_rows[1], int(T["d"][first_closed[1]])] = float("nan")
            (init if layout == AOS else init.t())[bad_rows[2], first_closed[2]] = float("nan")
            got = call(hm, q, qd, I, 10, layout, init=init)
            torch.cuda.synchronize()
            keep = torch.ones(B, dtype=torch.bool, device="cuda")
            keep[bad_rows] = False
            for g, w in zip(got, good):
                g, w = (g.reshape(B, -1), w.reshape(B, -1)) if layout == AOS or g.dim() == 1 else (g.t(), w.t())
                assert torch.isnan(g[bad_rows]).all(), f"layout={layout} {dtype}: a bad configuration has numbers in its outputs"
                assert not torch.isnan(w).any() and torch.equal(g[keep], w[keep]), f"layout={layout} {dtype}: a neighbour of a bad configuration changed"


_COVER = {}


def cover_reference(torch):
    if not _COVER:
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        sys_, desc, om = model_of("arm7")
        grid = 6 * cus  # limit_plan: six workgroups of (28 + 21) 64 doubles per CU
        B = 2 * grid * 64 + 64 + 37
        rows = DistinctRows(sys_, 256, seed=41)
        idx = group_cover(B, grid)
        q, qd, _, _ = rows.rows(idx)
        joints = jl.one_dof_joints(desc)
        R = jl.joint_limit_impulse(om, desc, q, qd, joints, [LOWER] * 7, [UPPER] * 7, MARGIN, ERP, 0.0, 4)
        _COVER.update(B=B, rows=rows, idx=idx, joints=joints, R=R, desc=desc)
    return _COVER


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the solve's grid holds, plus a ragged last group: every workgroup loops over several groups of 64.
    B distinct rows, poisoned outputs with guard rows, every row group checked, every entry written."""
    torch = torch_cuda
    C = cover_reference(torch)
    desc, B, idx, R = C["desc"], C["B"], C["idx"], C["R"]
    assert not R["bad"].any() and np.abs(np.abs(C["rows"].rows(idx)[0]) - 0.75).min() > 1.0e-9
    hm = hip_model(desc)
    q, qd, _, _ = C["rows"].device(torch, B)
    q, qd = laid_out(q, layout), laid_out(qd, layout)
    (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, 7, layout, torch.float64)
    hm.joint_limit_impulse(q, qd, C["joints"], [LOWER] * 7, [UPPER] * 7, MARGIN, ERP, iterations=4, layout=layout, out=(qdn, imp, res))
    torch.cuda.synchronize()
    tol = f32_aba_forward_factor(desc.n_joints) * U64 * float(R["cond_kkt"].max())
    check_cover(qdn_rows, qdn_guard, idx, R["qd_next"], tol, label=f"qd+ layout={layout}")
    check_cover(imp_rows, imp_guard, idx, R["impulse"], tol, label=f"impulse layout={layout}")
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
    q, qd = device_state(torch, I, B, AOS, torch.float64)
    ref = [t.clone() for t in call(hm, q, qd, I, 25, AOS)]
    torch.cuda.synchronize()
    views, streams = [hm.context(), hm.context()], [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[torch.zeros_like(t) for t in ref] for _ in views]
    for view in views:
        view.reserve(B)
    for view, s, o in zip(views, streams, outs):  # both in flight before either is waited for
        with torch.cuda.stream(s):
            call(view, q, qd, I, 25, AOS, tuple(o))
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
            call(view, q, qd, I, 25, AOS, tuple(o))
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
    q, qd = device_state(torch, I, B, layout, torch.float64)
    _, first, _ = call(hm, q, qd, I, 2, layout)
    start = first.clone()
    want = [t.clone() for t in call(hm, q, qd, I, 2, layout, init=start)]
    qdn, res = torch.empty_like(want[0]), torch.empty_like(want[2])
    call(hm, q, qd, I, 2, layout, (qdn, first, res), init=first)
    torch.cuda.synchronize()
    assert torch.equal(start, want[1]) is False  # two more sweeps moved the impulses
    for got, w in zip((qdn, first, res), want):
        assert torch.equal(got, w)


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 10
    lib = _lib.load()
    I = make_inputs(name, B)
    L = len(I["joints"])
    q, qd = dev(torch, I["q"]), dev(torch, I["qd"])
    init = torch.zeros((B, L), device="cuda", dtype=torch.float64)
    qdn, qdn_guard = poisoned(torch, B, (desc.nv,), torch.float64)
    imp, imp_guard = poisoned(torch, B, (L,), torch.float64)
    res, res_guard = poisoned(torch, B, (), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    jnt, lo, hi = np.array(I["joints"], dtype=np.int32), I["lower"].copy(), I["upper"].copy()
    floating = [j for j in range(desc.n_joints) if int(desc.joint_type[j]) == 2][0]
    arr = lambda values, dtype=np.float64: np.array(values, dtype=dtype)
    keep = dict(far=jnt.copy(), neg=jnt.copy(), root=jnt.copy(), twice=jnt.copy(), crossed=lo.copy(), nan_lo=lo.copy(), nan_hi=hi.copy())
    keep["far"][2], keep["neg"][0], keep["root"][1], keep["twice"][5] = desc.n_joints, -1, floating, jnt[0]
    keep["crossed"][3], keep["nan_lo"][0], keep["nan_hi"][L - 1] = 1.5, np.nan, np.nan

    def untouched(what, word=None):
        message = lib.mh_last_error().decode()
        assert message and (word is None or word in message), (what, message)
        for t in (qdn, qdn_guard, imp, imp_guard, res, res_guard):
            assert torch.isnan(t).all(), what

    def go(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), n=L, j=jnt.ctypes.data, lo=lo.ctypes.data, hi=hi.ctypes.data, margin=MARGIN, erp=ERP,
           init=init.data_ptr(), eps=0.0, it=10, out=qdn.data_ptr(), imp=imp.data_ptr(), res=res.data_ptr()):
        st = fn(hm._h, B, q, qd, n, j, lo, hi, margin, erp, init, eps, it, ctypes.byref(opts), out, imp, res)
        torch.cuda.synchronize()
        return st

    nan, inf = float("nan"), float("inf")
    refused = {"NULL q": (dict(q=None), "q"), "NULL qd": (dict(qd=None), "qd"), "NULL qd_out": (dict(out=None), "qd_out"),
               "NULL limit_joints": (dict(j=None), "limit_joints"), "NULL lower": (dict(lo=None), "lower"), "NULL upper": (dict(hi=None), "upper"),
               "no rows": (dict(n=0), "n_limits"), "too many rows": (dict(n=65), "n_limits"),
               "joint out of range": (dict(j=keep["far"].ctypes.data), "limit_joints[2]"), "negative joint": (dict(j=keep["neg"].ctypes.data), "limit_joints[0]"),
               "a floating joint": (dict(j=keep["root"].ctypes.data), "limit_joints[1]"), "listed twice": (dict(j=keep["twice"].ctypes.data), "limit_joints[5]"),
               "lower > upper": (dict(lo=keep["crossed"].ctypes.data), "lower"), "NaN lower": (dict(lo=keep["nan_lo"].ctypes.data), "lower"),
               "NaN upper": (dict(hi=keep["nan_hi"].ctypes.data), "upper"),
               "negative margin": (dict(margin=-1.0e-9), "margin"), "NaN margin": (dict(margin=nan), "margin"), "infinite margin": (dict(margin=inf), "margin"),
               "negative erp": (dict(erp=-1.0), "erp"), "NaN erp": (dict(erp=nan), "erp"), "infinite erp": (dict(erp=inf), "erp"),
               "negative compliance": (dict(eps=-1.0e-9), "compliance"), "NaN compliance": (dict(eps=nan), "compliance"),
               "infinite compliance": (dict(eps=inf), "compliance"), "no sweeps": (dict(it=0), "n_iterations"), "too many sweeps": (dict(it=4097), "n_iterations"),
               "qd_out is q": (dict(out=q.data_ptr()), "qd_out"), "qd_out is qd": (dict(out=qd.data_ptr()), "qd_out"),
               "impulse_out overlaps qd": (dict(imp=qd.data_ptr()), "impulse_out"),
               "impulse_out is part of impulse_init": (dict(imp=init.data_ptr() + 16, init=init.data_ptr()), "impulse_out"),
               "residual_out is impulse_init": (dict(res=init.data_ptr()), "residual_out"), "outputs overlap": (dict(imp=qdn.data_ptr() + 16), "impulse_out"),
               "residual_out inside impulse_out": (dict(res=imp.data_ptr() + 8), "residual_out")}
    for sfx in ("f64", "f32"):
        for what, (kw, word) in refused.items():
            assert go(getattr(lib, "mh_joint_limit_impulse_" + sfx), **kw) == INVALID, what
            untouched(what, word)
    before = [t.clone() for t in (q, qd, init)]
    assert go(lib.mh_joint_limit_impulse_f64, B=0) == 0 and go(lib.mh_joint_limit_impulse_f64, B=0, q=None, qd=None, out=None, imp=None, res=None) == 0
    untouched("B = 0")
    locked = hip_model(desc)
    modes = np.zeros(desc.n_joints, dtype=np.int32)
    modes[3] = 1
    locked.set_joint_source_modes(modes)
    assert lib.mh_joint_limit_impulse_f64(locked._h, B, q.data_ptr(), qd.data_ptr(), L, jnt.ctypes.data, lo.ctypes.data, hi.ctypes.data, MARGIN, ERP, None, 0.0, 10,
                                          ctypes.byref(opts), qdn.data_ptr(), imp.data_ptr(), res.data_ptr()) == INVALID
    untouched("acceleration-source joints", "acceleration sources")
    assert go(lib.mh_joint_limit_impulse_f64, it=4096, imp=None, res=None, eps=0.0, margin=0.0, erp=0.0) == 0  # the most sweeps, the optional outputs absent
    assert not torch.isnan(qdn).any() and torch.isnan(imp).all() and torch.isnan(res).all()
    assert go(lib.mh_joint_limit_impulse_f64, init=None) == 0
    for t, gd in ((qdn, qdn_guard), (imp, imp_guard), (res, res_guard)):
        assert not torch.isnan(t).any() and torch.isnan(gd).all()
    assert all(torch.equal(x, y) for x, y in zip((q, qd, init), before))
    with pytest.raises(_lib.MecanoHipError):
        hm.joint_limit_impulse(q, qd, I["joints"], lo[:3], hi)  # three lower limits for 24 joints
    with pytest.raises(_lib.MecanoHipError):
        hm.joint_limit_impulse(q, qd, I["joints"], lo, hi, init=init[:, :2].contiguous())
    with pytest.raises(ValueError):
        hm.joint_limit_impulse(q, qd, I["joints"], lo, hi, init=init.to(torch.float32))
