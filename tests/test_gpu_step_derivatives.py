"""mh_configuration_add_*, mh_configuration_difference_* and mh_aba_integrate_derivatives_* on the device against the CPU checker
(tests/step_derivatives_check.py, pinned by tests/test_step_derivatives_cpu.py), against the checker's assembly applied to the device's
own mh_aba_derivatives_* outputs (which isolates the new kernel), and against the library's own step."""
import functools

import numpy as np
import pytest

import helpers as hp
import step_derivatives_check as sc
from helpers import check_bad_outputs, close, close_aba, poisoned
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu

AOS, SOA = 0, 1
U64, U32 = 2.0 ** -53, 2.0 ** -24
TREE_ROWS = np.array([0, 1, 31, 63, 64, 69])  # (the checker takes seconds per row of the 128-body tree)
B70 = 70  # one full wave and a ragged one


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def soa(x):
    """[B, ...] -> [prod(...), B] contiguous"""
    return None if x is None else x.reshape(x.shape[0], -1).t().contiguous()


def state(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)


def host(t, layout, *shape):
    if t is None:
        return None
    a = (t.t() if layout == SOA else t).cpu().numpy().astype(np.float64)
    return a.reshape(shape)


def run_step(torch, hm, dt, q, qd, tau, f, layout, dtype=None):
    """(qdd, q_next, qd_next, A, B) as AoS-shaped fp64 numpy."""
    args = [dev(torch, x, dtype) for x in (q, qd, tau, f)]
    if layout == SOA:
        args = [soa(x) for x in args]
    out = hm.step_derivatives(dt, args[0], args[1], args[2], GRAVITY, args[3], layout)
    torch.cuda.synchronize()
    B, nv, nq = q.shape[0], hm.nv, hm.nq
    return (host(out[0], layout, B, nv), host(out[1], layout, B, nq), host(out[2], layout, B, nv), host(out[3], layout, B, 2 * nv, 2 * nv),
            host(out[4], layout, B, 2 * nv, nv))


def run_aba_derivatives(torch, hm, q, qd, tau, f, layout, dtype=None):
    args = [dev(torch, x, dtype) for x in (q, qd, tau, f)]
    if layout == SOA:
        args = [soa(x) for x in args]
    out = hm.aba_derivatives(args[0], args[1], args[2], GRAVITY, args[3], layout)
    torch.cuda.synchronize()
    B, nv = q.shape[0], hm.nv
    return (host(out[0], layout, B, nv),) + tuple(host(t, layout, B, nv, nv) for t in out[1:])


def inputs(case, B=B70, with_f=True):
    sys_, desc = make_case(case)
    q, qd, _, tau = state(sys_, B)
    f = random_wrenches(np.random.default_rng(31), B, desc.n_joints) if with_f else None
    return sys_, desc, q, qd, tau, f


@functools.lru_cache(maxsize=None)
def reference(case, dt, with_f):
    """The full checker's (qdd, A, B) and cond_inf(H) per row: computed once, shared by the layouts, never modified."""
    _, desc, q, qd, tau, f = inputs(case, with_f=with_f)
    ref = sc.step_derivatives(desc, dt, q, qd, tau, GRAVITY, f)
    conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(q)])
    return ref, conds


def isolated_kernel_ratio(m, dt, qd, qdd, Dq, Dv, Hinv, A, Bm, rows, u):
    """Worst |device - assembly of the device's own derivative matrices| / (24 u x the per-entry sum of absolute terms)."""
    worst = 0.0
    for b in rows:
        Ar, Br, Aa, Ba = sc.assemble_one(m, dt, qd[b], qdd[b], Dq[b], Dv[b], Hinv[b])
        for got, ref, ab in ((A[b], Ar, Aa), (Bm[b], Br, Ba)):
            err, bound = np.abs(got - ref), 24.0 * u * ab
            assert np.all(err[bound == 0.0] == 0.0)  # entries no term goes into are exact zeros
            worst = max(worst, float((err[bound > 0.0] / bound[bound > 0.0]).max()))
    return worst


# ------------------------------------------------------------------------------------------------ the linearisation
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("dt", [0.1, 1.0e-3])
def test_fp64_matches_checker(torch_cuda, case, layout, dt):
    """Every model of the CPU pins, both layouts, dt = 0.1 (J_r and E far from the identity) and 1e-3, f_ext with AoS.  (1) against the
    checker's assembly of the device's own mh_aba_derivatives_f64 outputs: 24 u x the sum of the absolute terms of the entry -- pure
    rounding of about twenty products.  (2) against the full checker: 8 sqrt(8 (3 n + 1)) cond_inf(H) u max(1, |ref|_inf), helpers.close_aba
    with one more combination step than the forward-dynamics derivatives.  (3) qdd, q_next, qd_next are mh_aba_f64 + mh_integrate_f64."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    with_f = layout == AOS
    sys_, desc, q, qd, tau, f = inputs(case, with_f=with_f)
    hm, m, B = HipModel(desc), sc.StepModel(desc), B70
    qdd, qn, vn, A, Bm = run_step(torch, hm, dt, q, qd, tau, f, layout)
    for x in (qdd, qn, vn, A, Bm):
        assert not np.isnan(x).any()
    qdd_d, Dq, Dv, Hinv = run_aba_derivatives(torch, hm, q, qd, tau, f, layout)
    ratio = isolated_kernel_ratio(m, dt, qd, qdd_d, Dq, Dv, Hinv, A, Bm, range(B), U64)
    print(f"{case} layout {layout} dt {dt}: assembly kernel, worst err / (24 u abs-sum) = {ratio:.3e}")
    assert ratio <= 1.0
    (qdd_ref, A_ref, B_ref), conds = reference(case, dt, with_f)
    n3 = 3 * desc.n_joints + 1
    close_aba(A.reshape(B, -1), A_ref.reshape(B, -1), None, n3, U64, label=f"A layout {layout}", conds=conds)
    close_aba(Bm.reshape(B, -1), B_ref.reshape(B, -1), None, n3, U64, label=f"B layout {layout}", conds=conds)
    # the step itself: forward dynamics and the integrator issued the same way
    a = [dev(torch, x) for x in (q, qd, tau, f)]
    if layout == SOA:
        a = [soa(x) for x in a]
    qdd_dev = hm.aba(a[0], a[1], a[2], GRAVITY, a[3], layout)
    qn_dev, vn_dev = hm.integrate(dt, a[0], a[1], qdd_dev, layout)
    torch.cuda.synchronize()
    got = (qdd, qn, vn)
    want = (host(qdd_dev, layout, B, hm.nv), host(qn_dev, layout, B, hm.nq), host(vn_dev, layout, B, hm.nv))
    if not all(np.array_equal(g, w) for g, w in zip(got, want)):  # (forward dynamics may take another plan beside other launches)
        for g, w, name in zip(got, want, ("qdd", "q_next", "qd_next")):
            close_aba(g, w, None, desc.n_joints, U64, label=f"{name} vs aba + integrate", conds=conds)


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_fp32_matches_checker_across_the_series_switch(torch_cuda, case):
    """fp32, both layouts, dt in {0, 1e-6, 1e-3, 0.1}: the coefficients of J_r on both sides of their series switch and at the step's own
    identity threshold.  Against the fp64 checker on the fp32-rounded inputs with test_forward_fp32_matches_checker's bound (close_aba, u =
    2^-24, one more combination step); no NaN anywhere."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc, q, qd, tau, f = inputs(case, B=B70)
    q, qd, tau, f = (x.astype(np.float32) for x in (q, qd, tau, f))
    hm, B = HipModel(desc), B70
    q64, qd64, tau64, f64 = (x.astype(np.float64) for x in (q, qd, tau, f))
    conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(q64)])
    m = sc.StepModel(desc)
    base = [sc.dc.aba_derivatives_one(m, q64[b], qd64[b], tau64[b], GRAVITY, f64[b]) for b in range(B)]
    n3 = 3 * desc.n_joints + 1
    for dt in (0.0, 1.0e-6, 1.0e-3, 0.1):
        ref = [sc.assemble_one(m, dt, qd64[b], *base[b]) for b in range(B)]
        A_ref, B_ref = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        for layout in (AOS, SOA):
            out = run_step(torch, hm, dt, q, qd, tau, f, layout, dtype=torch.float32)
            for x in out:
                assert not np.isnan(x).any()
            close_aba(out[3].reshape(B, -1), A_ref.reshape(B, -1), None, n3, U32, label=f"fp32 A dt {dt} layout {layout}", conds=conds)
            close_aba(out[4].reshape(B, -1), B_ref.reshape(B, -1), None, n3, U32, label=f"fp32 B dt {dt} layout {layout}", conds=conds)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_zero_step_is_exactly_the_identity(torch_cuda, dtype_name, layout):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    for case in ("humanoid30", "planar", "spherical"):
        sys_, desc, q, qd, tau, f = inputs(case)
        np_dt = np.float32 if dtype == torch.float32 else np.float64
        out = run_step(torch, HipModel(desc), 0.0, *(x.astype(np_dt) for x in (q, qd, tau, f)), layout, dtype=dtype)
        assert np.array_equal(out[3], np.broadcast_to(np.eye(2 * desc.nv), out[3].shape)) and not out[4].any()


def test_tree_beyond_what_lds_holds(torch_cuda):
    """The committed 128-body benchmark tree, nv = 323: no matrix fits LDS, the assembly streams rows; two chunks of joints."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_ = rt.committedBenchmarkSystems()["tree128"]
    desc = sys_.toModelDesc()
    assert desc.nv == 323
    hm, m, B, dt = HipModel(desc), sc.StepModel(desc), B70, 0.01
    q, qd, _, tau = state(sys_, B)
    f = random_wrenches(np.random.default_rng(31), B, desc.n_joints)
    qdd, qn, vn, A, Bm = run_step(torch, hm, dt, q, qd, tau, f, AOS)
    assert not any(np.isnan(x).any() for x in (qdd, qn, vn, A, Bm))
    qdd_d, Dq, Dv, Hinv = run_aba_derivatives(torch, hm, q, qd, tau, f, AOS)
    ratio = isolated_kernel_ratio(m, dt, qd, qdd_d, Dq, Dv, Hinv, A, Bm, TREE_ROWS, U64)
    print(f"tree128: assembly kernel, worst err / (24 u abs-sum) = {ratio:.3e}")
    assert ratio <= 1.0
    _, A_ref, B_ref = sc.step_derivatives(m, dt, q, qd, tau, GRAVITY, f, rows=TREE_ROWS)
    H = OracleModel(desc).crba(q[TREE_ROWS])
    n3, R = 3 * desc.n_joints + 1, len(TREE_ROWS)
    close_aba(A[TREE_ROWS].reshape(R, -1), A_ref[TREE_ROWS].reshape(R, -1), H, n3, U64, label="tree A")
    close_aba(Bm[TREE_ROWS].reshape(R, -1), B_ref[TREE_ROWS].reshape(R, -1), H, n3, U64, label="tree B")


@pytest.mark.parametrize("skip", ["none", "qdd", "next", "A", "B"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_each_output_null_in_turn_nothing_else_written(torch_cuda, skip, layout):
    """Poisoned outputs with a guard row behind each: every entry inside is written, nothing behind; what is given has the bits of the
    call with every output."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc, q, qd, tau, f = inputs("humanoid30", B=64 * 3 + 5)
    hm, B, nv, nq = HipModel(desc), 64 * 3 + 5, desc.nv, desc.nq
    a = [dev(torch, x) for x in (q, qd, tau, f)]
    if layout == SOA:
        a = [soa(x) for x in a]
    full = hm.step_derivatives(0.01, a[0], a[1], a[2], GRAVITY, a[3], layout)
    shapes = [(nv,), (nq,), (nv,), (2 * nv, 2 * nv), (2 * nv, nv)]
    gone = {"none": (), "qdd": (0,), "next": (1, 2), "A": (3,), "B": (4,)}[skip]
    outs, guards = [], []
    for k, s in enumerate(shapes):
        if k in gone:
            outs.append(None), guards.append(None)
            continue
        o, g = poisoned(torch, B, s, torch.float64) if layout == AOS else poisoned(torch, int(np.prod(s)), (B,), torch.float64)
        outs.append(o), guards.append(g)
    hm.step_derivatives(0.01, a[0], a[1], a[2], GRAVITY, a[3], layout, out=tuple(outs))
    torch.cuda.synchronize()
    for k, (o, g, r) in enumerate(zip(outs, guards, full)):
        if o is None:
            continue
        assert torch.isnan(g).all(), f"output {k}: wrote past the end"
        assert not torch.isnan(o).any(), f"output {k}: entries left unwritten"
        if k >= 3:  # the matrices: the same launches on the same inputs
            assert torch.equal(o, r), f"output {k}"
        else:
            close_aba(host(o, layout, B, -1), host(r, layout, B, -1), OracleModel(desc).crba(q), desc.n_joints, U64, label=f"output {k}")


def test_rows_and_columns_of_unowned_indices_are_zero(torch_cuda):
    """A custom index map with two DoF / configuration indices no joint owns: their rows and columns of A and B are written as zeros, q_next
    and qd_next are not written there, and the rest is the default map's matrices."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, d0 = make_case("onedof_tree")
    q, qd, _, tau = state(sys_, B70)
    nv = d0.nv
    place = np.array([k + (k >= 3) + (k >= 7) for k in range(nv)])  # indices 3 and 8 of the wide map stay free
    free = np.setdiff1d(np.arange(nv + 2), place)
    d1 = sys_.toModelDesc()
    d1.dof_indices = place[np.asarray(d0.dof_indices)].astype(np.int32)
    d1.cfg_indices = place[np.asarray(d0.cfg_indices)].astype(np.int32)
    d1.nv = d1.nq = nv + 2
    wide = lambda x: np.ascontiguousarray(np.insert(np.insert(x, 3, 0.25, axis=1), 8, -0.5, axis=1))
    assert np.array_equal(wide(q)[:, place], q)
    base = run_step(torch, HipModel(d0), 0.05, q, qd, tau, None, AOS)
    conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(d0).crba(q)])
    for layout in (AOS, SOA):
        hm = HipModel(d1)
        a = [dev(torch, wide(x)) for x in (q, qd, tau)]
        outs = [poisoned(torch, B70, s, torch.float64)[0] for s in ((nv + 2,), (nv + 2,), (nv + 2,), (2 * nv + 4, 2 * nv + 4), (2 * nv + 4, nv + 2))]
        if layout == SOA:
            a, outs = [soa(x) for x in a], [soa(x) for x in outs]
        hm.step_derivatives(0.05, a[0], a[1], a[2], GRAVITY, None, layout, out=tuple(outs))
        torch.cuda.synchronize()
        qdd, qn, vn = (host(t, layout, B70, nv + 2) for t in outs[:3])
        A, Bm = host(outs[3], layout, B70, 2 * nv + 4, 2 * nv + 4), host(outs[4], layout, B70, 2 * nv + 4, nv + 2)
        assert np.isnan(qn[:, free]).all() and np.isnan(vn[:, free]).all()  # entries no joint owns are not written
        free2, place2 = np.concatenate([free, nv + 2 + free]), np.concatenate([place, nv + 2 + place])
        assert not A[:, free2, :].any() and not A[:, :, free2].any() and not Bm[:, free2, :].any() and not Bm[:, :, free].any()
        n3 = 3 * d0.n_joints + 1
        close_aba(A[:, place2][:, :, place2].reshape(B70, -1), base[3].reshape(B70, -1), None, n3, U64, label="A, wide map", conds=conds)
        close_aba(Bm[:, place2][:, :, place].reshape(B70, -1), base[4].reshape(B70, -1), None, n3, U64, label="B, wide map", conds=conds)
        # and the chart calls on the same map: unowned DoF entries of the difference are written as 0, of the sum not at all
        dq = torch.full_like(a[1], float("nan"))
        hm.configuration_difference(a[0], a[0], layout, out=dq)
        assert not dq.any()
        qo = torch.full_like(a[0], float("nan"))
        hm.configuration_add(a[0], a[1], layout, out=qo)
        qo = host(qo, layout, B70, nv + 2)
        assert np.isnan(qo[:, free]).all() and not np.isnan(qo[:, place]).any()


# ------------------------------------------------------------------------------------------------ the chart
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_chart_matches_checker_round_trip_and_in_place(torch_cuda, case, layout):
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, m, B = HipModel(desc), sc.StepModel(desc), B70
    q0, q1 = state(sys_, B, 5)[0], state(sys_, B, 6)[0]
    dq = np.random.default_rng(3).uniform(-1.0, 1.0, (B, desc.nv))
    dq[0] *= 1.0e-9
    lay = (lambda x: soa(x)) if layout == SOA else (lambda x: x)
    tq0, tq1, tdq = lay(dev(torch, q0)), lay(dev(torch, q1)), lay(dev(torch, dq))
    added = hm.configuration_add(tq0, tdq, layout)
    diff = hm.configuration_difference(tq0, tq1, layout)
    back = hm.configuration_difference(tq0, added, layout)
    again = hm.configuration_add(tq0, diff, layout)
    same = hm.configuration_difference(tq1, again, layout)
    in_place = tq0.clone()
    assert hm.configuration_add(in_place, tdq, layout, out=in_place) is in_place
    torch.cuda.synchronize()
    assert torch.equal(in_place, added)
    close(host(added, layout, B, desc.nq), sc.configuration_add(m, q0, dq), 1.0e-13, absolute=True, label="add")
    close(host(diff, layout, B, desc.nv), sc.configuration_difference(m, q0, q1), 1.0e-13, absolute=True, label="difference")
    close(host(back, layout, B, desc.nv), dq, 1.0e-12, absolute=True, label="(q (+) dq) (-) q")
    close(host(same, layout, B, desc.nv), np.zeros((B, desc.nv)), 1.0e-12, absolute=True, label="q0 (+) (q1 (-) q0) is q1")
    if layout == AOS:  # fp32 runs and stays finite
        f32 = hm.configuration_difference(tq0.float(), hm.configuration_add(tq0.float(), tdq.float()))
        close(f32.cpu().numpy().astype(np.float64), dq, 64 * U32 * 4.0, absolute=True, label="fp32 round trip")


def test_the_librarys_own_step_is_what_is_linearised(torch_cuda):
    """One rotational column of the floating joint of the humanoid: configuration_difference(step(x), step(x (+) eps e)) / eps and the
    plain difference of qd_next, eps = 1e-6, against A e within 2e-5 cond_inf(H) max(1, |A|_inf) -- all on the device."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc, q, qd, tau, _ = inputs("humanoid30", with_f=False)
    hm, m, B, dt, eps = HipModel(desc), sc.StepModel(desc), B70, 0.05, 1.0e-6
    floating = [i for i in range(m.n) if int(m.type[i]) == sc.SIXDOF][0]
    tq, tqd, ttau = dev(torch, q), dev(torch, qd), dev(torch, tau)
    _, qn, vn, A, _ = hm.step_derivatives(dt, tq, tqd, ttau, GRAVITY)
    conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(q)])
    for col in (int(m.dofs(floating)[1]), int(m.dofs(floating)[4])):
        e = torch.zeros_like(tqd)
        e[:, col] = eps
        q_eps = hm.configuration_add(tq, e)
        qn_eps, vn_eps = hm.integrate(dt, q_eps, tqd, hm.aba(q_eps, tqd, ttau, GRAVITY))
        lhs = torch.cat([hm.configuration_difference(qn, qn_eps), vn_eps - vn], dim=1) / eps
        torch.cuda.synchronize()
        err = (lhs - A[:, :, col]).abs().amax(dim=1).cpu().numpy()
        bound = 2.0e-5 * conds * np.maximum(1.0, A.abs().amax(dim=(1, 2)).cpu().numpy())
        print(f"column {col}: worst err / bound {float((err / bound).max()):.3e}")
        assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------ plumbing
def test_context_on_its_own_stream_and_graph_replay(torch_cuda):
    """A context view on a non-default stream gives the default context's bits; after reserve() and one first call the three calls are
    captured into a graph (they allocate nothing) and the replay gives the bits of the direct call, also on new inputs."""
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, dt = HipModel(desc), 1000, 0.01
    q, qd, _, tau = (dev(torch, x) for x in state(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    dq = dev(torch, np.random.default_rng(4).uniform(-0.5, 0.5, (B, desc.nv)))

    def direct(model, q_):
        step = model.step_derivatives(dt, q_, qd, tau, GRAVITY, f)
        added = model.configuration_add(q_, dq)
        return step + (added, model.configuration_difference(q_, added))

    ref = direct(hm, q)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    out = tuple(torch.empty_like(t) for t in ref)

    def issue():
        view.step_derivatives(dt, q, qd, tau, GRAVITY, f, out=(None,) + out[1:5])  # qdd in the context's scratch
        view.configuration_add(q, dq, out=out[5])
        view.configuration_difference(q, out[5], out=out[6])

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        issue()
        view.check(s.cuda_stream)
        assert all(torch.equal(a, b) for a, b in zip(out[1:], ref[1:]))
        for t in out:
            t.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            issue()
    torch.cuda.synchronize()
    assert not any(t.any() for t in out)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out[1:], ref[1:]))
    q2 = dev(torch, state(sys_, B, seed=6)[0])
    ref2 = direct(hm, q2)
    q.copy_(q2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out[1:], ref2[1:]))
    view.close()


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, nq, n = HipModel(desc), 10, desc.nv, desc.nq, desc.n_joints
    q, qd, _, tau = (dev(torch, x) for x in state(sys_, B))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    outs = lambda: (nan(B, nv), nan(B, nq), nan(B, nv), nan(B, 2 * nv, 2 * nv), nan(B, 2 * nv, nv))
    untouched = lambda o: all(torch.isnan(t).all() for t in o if t is not None)
    # shapes
    for bad in ((z(B, nv + 1),) + outs()[1:], outs()[:3] + (z(B, 2 * nv, nv), None), outs()[:4] + (z(B, nv, 2 * nv),), outs()[:4],
                outs()[:3] + (z(4 * nv * nv, B), None)):
        with pytest.raises(_lib.MecanoHipError):
            hm.step_derivatives(0.01, q, qd, tau, GRAVITY, None, out=bad)
    for bad_f in (z(B, n - 1, 6), z(B + 1, n, 6)):
        with pytest.raises(_lib.MecanoHipError):
            hm.step_derivatives(0.01, q, qd, tau, GRAVITY, bad_f)
    check_bad_outputs(torch, [(B, nv), (B, nq), (B, nv), (B, 2 * nv, 2 * nv), (B, 2 * nv, nv)],
                      lambda out: hm.step_derivatives(0.01, q, qd, tau, GRAVITY, None, out=out))
    check_bad_outputs(torch, (B, nq), lambda out: hm.configuration_add(q, qd, out=out))
    check_bad_outputs(torch, (B, nv), lambda out: hm.configuration_difference(q, q.clone(), out=out))
    with pytest.raises(_lib.MecanoHipError):
        hm.configuration_add(q, z(B, nv + 1))
    with pytest.raises(_lib.MecanoHipError):
        hm.configuration_difference(q, z(B, nq + 1))
    # what the C-ABI refuses, before any launch
    o = outs()
    for bad in ((None, None, None, None, None), (None, o[1], None, o[3], None), (None, None, o[2], o[3], None)):
        with pytest.raises(_lib.MecanoHipError) as ei:
            hm.step_derivatives(0.01, q, qd, tau, GRAVITY, None, out=bad)
        assert ei.value.status == 1 and untouched(bad)
    for bad_dt in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.MecanoHipError) as ei:
            hm.step_derivatives(bad_dt, q, qd, tau, GRAVITY, None, out=o)
        assert ei.value.status == 1 and untouched(o)
    hm.step_derivatives(-0.01, q, qd, tau, GRAVITY)  # a negative step is a step
    big = nan(B * 4 * nv * nv + B * nv)
    part = lambda ofs, *shape: big[ofs: ofs + int(np.prod(shape))].view(*shape)
    overlaps = [(None, q, qd, o[3], o[4]),  # the in-place step is refused here
                (qd, None, None, o[3], None), (tau, None, None, o[3], None),
                (None, None, None, part(0, B, 2 * nv, 2 * nv), part(8, B, 2 * nv, nv)), (part(0, B, nv), None, None, part(4, B, 2 * nv, 2 * nv), None)]
    for bad in overlaps:
        with pytest.raises(_lib.MecanoHipError) as ei:
            hm.step_derivatives(0.01, q, qd, tau, GRAVITY, None, out=bad)
        assert ei.value.status == 1
    assert torch.isnan(big).all() and untouched(o)
    with pytest.raises(_lib.MecanoHipError):
        hm.configuration_add(q, qd, out=qd)
    with pytest.raises(_lib.MecanoHipError):
        hm.configuration_difference(q, q.clone(), out=q)
    # locked joints
    modes = np.zeros(n, dtype=np.int32)
    modes[2] = 1
    hm.set_joint_source_modes(modes)
    with pytest.raises(_lib.MecanoHipError) as ei:
        hm.step_derivatives(0.01, q, qd, tau, GRAVITY, None, out=o)
    assert ei.value.status == 1 and untouched(o)
    hm.set_joint_source_modes(None)
    # B = 0 touches nothing
    e = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    hm.step_derivatives(0.01, e(0, nq), e(0, nv), e(0, nv), GRAVITY)
    assert hm.configuration_add(e(0, nq), e(0, nv)).shape == (0, nq) and hm.configuration_difference(e(0, nq), e(0, nq)).shape == (0, nv)
    torch.cuda.synchronize()


def test_calculator_mirror(torch_cuda):
    from mecano_amd.calculators import ForwardDynamicsCalculator
    from mecano_amd.engine import HipModel
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    B = 40
    q, qd, _, tau = (dev(torch, x) for x in state(sys_, B))
    f = dev(torch, random_wrenches(np.random.default_rng(27), B, desc.n_joints, always=True))
    fwd = ForwardDynamicsCalculator(sys_)
    fwd.setGravitationalAcceleration(*GRAVITY)
    fwd.setExternalWrenches(f)
    got = fwd.getStepLinearization(0.02, q, qd, tau)
    want = HipModel(desc).step_derivatives(0.02, q, qd, tau, GRAVITY, f)
    torch.cuda.synchronize()
    conds = np.array([np.linalg.cond(h, np.inf) for h in OracleModel(desc).crba(q.cpu().numpy())])
    for g, w in zip(got, want):
        if not torch.equal(g, w):  # (two models: forward dynamics may take another plan)
            close_aba(g.cpu().numpy().reshape(B, -1), w.cpu().numpy().reshape(B, -1), None, 3 * desc.n_joints + 1, U64, conds=conds)


# ------------------------------------------------------------------------------------------------ scattered index maps
SCATTERED_DT = 0.05


@functools.lru_cache(maxsize=None)
def _scattered_reference(model, dtype_name):
    """States in the identity description's index space, the checker's (qdd, A, B) on them, the oracle's step and cond_inf(H) per row:
    once per model and precision, shared by the layouts and the hole cases, never modified."""
    sys_, d0 = hp.SCATTERED_MODELS[model]()
    np_dt = np.float32 if dtype_name == "float32" else np.float64
    q, qd, _, tau = hp.DistinctRows(sys_, 16, seed=45).rows(np.arange(B70), np_dt)
    f = random_wrenches(np.random.default_rng(46), B70, d0.n_joints).astype(np_dt).astype(np.float64)
    qdd, A, Bm = sc.step_derivatives(d0, SCATTERED_DT, q, qd, tau, GRAVITY, f)
    om = OracleModel(d0)
    qn, vn = om.integrate(SCATTERED_DT, q, qd, qdd)[:2]
    conds = np.array([np.linalg.cond(h, np.inf) for h in om.crba(q)])
    assert conds.max() < 1.0e8
    return (q, qd, tau, f), (qdd, qn, vn, A, Bm), conds


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_scattered_index_maps(torch_cuda, model, holes, layout, dtype_name):
    """step_derivatives on a description whose maps send every DoF and every configuration entry somewhere else (with holes: two indices
    of each space owned by no joint, holding 7.0 in every input), on moved states, against the checker on the IDENTITY description.  A and B
    go back through both copies of the DoF space stacked in them, q_next through the configuration map, qdd and qd_next through the DoF map;
    bounds: test_fp64_matches_checker's / the fp32 test's (close_aba, 3 n + 1 for the matrices, n for the vectors).  Rows and columns of
    unowned indices are exact zeros, unowned entries of q_next / qd_next are not written, the guard rows stay poisoned; with the rows or
    the columns left where they are A and B miss the reference by more than 1e-3; at dt = 0 A is the identity on the owned indices and B
    is zero, exactly."""
    torch = torch_cuda
    dtype, u = getattr(torch, dtype_name), (U32 if dtype_name == "float32" else U64)
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, B, nv, nq, n = hp.scattered_model(d, model), B70, d.nv, d.nq, d0.n_joints
    (q, qd, tau, f), ref, conds = _scattered_reference(model, dtype_name)
    is_soa = layout == SOA
    lay = soa if is_soa else (lambda x: x)
    tq, tqd, ttau = (lay(dev(torch, x, dtype)) for x in (hp.to_q(q, pq, nq), hp.to_v(qd, pv, nv), hp.to_v(tau, pv, nv)))
    tf = lay(dev(torch, f, dtype))
    shapes = [(nv,), (nq,), (nv,), (2 * nv, 2 * nv), (2 * nv, nv)]
    free_v, free_q = hp.unowned(pv, nv), hp.unowned(pq, nq)
    for dt in (SCATTERED_DT, 0.0):
        outs, guards = hp.poisoned_set(torch, B, shapes, dtype, is_soa)
        hm.step_derivatives(dt, tq, tqd, ttau, GRAVITY, tf, layout, out=tuple(outs))
        torch.cuda.synchronize()
        hp.guards_intact(guards, f"step_derivatives dt {dt}")
        qdd, qn, vn, A, Bm = (hp.rows_of(o, B, s, is_soa) for o, s in zip(outs, shapes))
        assert np.isnan(qn[:, free_q]).all() and np.isnan(vn[:, free_v]).all()  # entries no joint owns are not written
        (A_back, A_rows, A_cols), (B_back, B_rows, B_cols) = hp.from_step(A, pv), hp.from_step(Bm, pv)
        assert not A_rows.any() and not A_cols.any() and not B_rows.any() and not B_cols.any()  # exact zeros, and written
        if dt == 0.0:
            assert np.array_equal(A_back, np.broadcast_to(np.eye(2 * d0.nv), A_back.shape)) and not B_back.any()
            assert np.array_equal(hp.from_v(vn, pv)[0], qd.astype(np.float32 if dtype_name == "float32" else np.float64))
            continue
        close_aba(hp.from_v(qdd, pv)[0], ref[0], None, n, u, label="scattered qdd", conds=conds)
        close_aba(hp.from_v(qn, pq)[0], ref[1], None, n, u, label="scattered q_next", conds=conds)
        close_aba(hp.from_v(vn, pv)[0], ref[2], None, n, u, label="scattered qd_next", conds=conds)
        close_aba(A_back.reshape(B, -1), ref[3].reshape(B, -1), None, 3 * n + 1, u, label="scattered A", conds=conds)
        close_aba(B_back.reshape(B, -1), ref[4].reshape(B, -1), None, 3 * n + 1, u, label="scattered B", conds=conds)
        hp.assert_misses(hp.keep_order(qn, pq), ref[1], "q_next")
        hp.assert_misses(hp.keep_order(vn, pv), ref[2], "qd_next")
        for M, r, name in ((A, ref[3], "A"), (Bm, ref[4], "B")):
            hp.assert_misses(hp.keep_order_step(M, pv, rows=True, cols=False), r, f"{name}, rows left where they are")
            hp.assert_misses(hp.keep_order_step(M, pv, rows=False, cols=True), r, f"{name}, columns left where they are")


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("model,holes", hp.SCATTERED_CASES)
def test_chart_on_scattered_index_maps(torch_cuda, model, holes, layout):
    """configuration_add (into a fresh output and onto q itself) and configuration_difference on scattered maps against the checker on the
    IDENTITY description, test_chart_matches_checker_round_trip_and_in_place's 1e-13 absolute; unowned entries of the difference are
    exact zeros, of the sum not written; read without moving them back both miss the reference by more than 1e-3.  fp32: the round trip
    (q (+) dq) (-) q = dq of that test under its 64 * 4 * 2^-24 absolute, and the sum against the checker on the fp32-rounded inputs under
    the same figure (an entry of the sum is one rotation and one addition on |q| <= 4: a few u |q|, far inside it)."""
    torch = torch_cuda
    sys_, d0, d, pv, pq = hp.scattered_case(model, holes)
    hm, m0, B, nv, nq = hp.scattered_model(d, model), sc.StepModel(d0), B70, d.nv, d.nq
    rows = hp.DistinctRows(sys_, 16, seed=47)
    q0, q1 = rows.rows(np.arange(B))[0], rows.rows(np.arange(B, 2 * B))[0]
    dq = np.random.default_rng(48).uniform(-1.0, 1.0, (B, d0.nv))
    dq[0] *= 1.0e-9
    is_soa = layout == SOA
    lay = soa if is_soa else (lambda x: x)
    tq0, tq1, tdq = (lay(dev(torch, x)) for x in (hp.to_q(q0, pq, nq), hp.to_q(q1, pq, nq), hp.to_v(dq, pv, nv)))
    (added, diff), guards = hp.poisoned_set(torch, B, [(nq,), (nv,)], torch.float64, is_soa)
    hm.configuration_add(tq0, tdq, layout, out=added)
    hm.configuration_difference(tq0, tq1, layout, out=diff)
    in_place = tq0.clone()
    assert hm.configuration_add(in_place, tdq, layout, out=in_place) is in_place
    torch.cuda.synchronize()
    hp.guards_intact(guards, "chart")
    added, diff, in_place = hp.rows_of(added, B, (nq,), is_soa), hp.rows_of(diff, B, (nv,), is_soa), hp.rows_of(in_place, B, (nq,), is_soa)
    add_ref, diff_ref = sc.configuration_add(m0, q0, dq), sc.configuration_difference(m0, q0, q1)
    (add_back, add_free), (diff_back, diff_free), (place_back, place_free) = hp.from_v(added, pq), hp.from_v(diff, pv), hp.from_v(in_place, pq)
    assert np.isnan(add_free).all() and not diff_free.any() and np.all(place_free == hp.UNOWNED)
    close(add_back, add_ref, 1.0e-13, absolute=True, label="scattered add")
    close(diff_back, diff_ref, 1.0e-13, absolute=True, label="scattered difference")
    assert np.array_equal(place_back, add_back)
    hp.assert_misses(hp.keep_order(added, pq), add_ref, "add")
    hp.assert_misses(hp.keep_order(diff, pv), diff_ref, "difference")
    # fp32 (mh_configuration_add_f32 / _difference_f32 read both maps too): that test's round trip (q (+) dq) (-) q = dq within its
    # 64 * 4 u absolute, on the scattered description, and the sum itself against the checker on the fp32-rounded inputs to the same bound
    f32 = torch.float32
    q32, dq32 = q0.astype(np.float32).astype(np.float64), dq.astype(np.float32).astype(np.float64)
    sq, sdq = lay(dev(torch, hp.to_q(q32, pq, nq), f32)), lay(dev(torch, hp.to_v(dq32, pv, nv), f32))
    (added32, back32), guards = hp.poisoned_set(torch, B, [(nq,), (nv,)], f32, is_soa)
    hm.configuration_add(sq, sdq, layout, out=added32)
    torch.cuda.synchronize()
    assert np.isnan(hp.from_v(hp.rows_of(added32, B, (nq,), is_soa), pq)[1]).all()  # unowned entries of the sum are not written
    (added32 if not is_soa else added32.t())[:, torch.as_tensor(hp.unowned(pq, nq), device="cuda")] = hp.UNOWNED  # (an input next: finite there)
    hm.configuration_difference(sq, added32, layout, out=back32)
    torch.cuda.synchronize()
    hp.guards_intact(guards, "fp32 chart")
    added32, back32 = hp.rows_of(added32, B, (nq,), is_soa), hp.rows_of(back32, B, (nv,), is_soa)
    trip, trip_free = hp.from_v(back32, pv)
    assert not trip_free.any() and not np.isnan(trip).any()
    close(trip, dq32, 64 * U32 * 4.0, absolute=True, label="scattered fp32 round trip")
    close(hp.from_v(added32, pq)[0], sc.configuration_add(m0, q32, dq32), 64 * U32 * 4.0, absolute=True, label="scattered fp32 add")
    hp.assert_misses(hp.keep_order(back32, pv), dq32, "fp32 round trip")
    hp.assert_misses(hp.keep_order(added32, pq), sc.configuration_add(m0, q32, dq32), "fp32 add")
