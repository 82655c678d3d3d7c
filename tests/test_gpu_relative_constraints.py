"""mh_aba_constrained_between_* and mh_constraint_impulse_between_* on the device against the dense KKT checker
(tests/relative_constraints_check.py, pinned by tests/test_relative_constraints_cpu.py), through the C-ABI (HipModel.aba_constrained /
constraint_impulse with ``bases`` are the ctypes calls).  Every output is poisoned and has a guard row behind it.

The bound is helpers.close_aba applied to the matrix actually solved: per configuration
    |x - ref|_inf <= f32_aba_forward_factor(n_joints) cond_inf(KKT of the reference) u max(1, |ref|_inf),   x = (qdd, lambda),
u = 2^-53 or 2^-24; fp32 is held against the fp64 checker on the fp32-rounded inputs.  In fp32 that bound is near 0.7 max(1, |ref|_inf) at
cond 1e5, so the two residuals held beside it with cond_inf(H) in its place are the check that bites there: the constraint equation
through the checker's J and c, and the equation of motion (impulse: the momentum balance) through the oracle's inverse dynamics under the
equal-and-opposite wrenches."""
import ctypes

import numpy as np
import pytest

import helpers as hp
import kinematics_check as kc
import relative_constraints_check as rc
from helpers import DistinctRows, U32, check_cover, close, close_aba, f32_aba_forward_factor, group_cover, poisoned
from oracle.cpu_oracle import OracleModel
from test_constrained_dynamics_cpu import GRAVITY
from test_gpu_constrained_dynamics import (AOS, BATCHES, B_MAX, INVALID, SOA, U64, check_exact_zeros, dev, hip_model, hold_residual, laid_out,
                                           moved_inputs, outputs, scattered_description, torch_cuda)  # noqa: F401 (torch_cuda is a fixture)
from test_relative_constraints_cpu import (CASES, P_BASES, P_GRAVITY, P_POSES, P_ROWS, P_TARGETS, make_inputs, model_of, parallelogram,
                                           parallelogram_state, reference, reference_impulse)

pytestmark = pytest.mark.gpu

_REFS = {}


def references(name, dtype_name):
    """(inputs, checker result of the accelerations, of the impulse) of B_MAX configurations, once per (case, precision); a smaller batch
    takes the first rows.  fp32: the checker runs in fp64 on the fp32-rounded inputs."""
    key = (name, dtype_name)
    if key not in _REFS:
        I = make_inputs(name, B_MAX, dtype=np.float64 if dtype_name == "f64" else np.float32)
        R = reference(name, I)
        _REFS[key] = (I, R, reference_impulse(name, I, terms=R))
    return _REFS[key]


def device_inputs(torch, I, B, layout, dtype):
    d = {k: laid_out(dev(torch, I[k][:B], dtype), layout) for k in ("q", "qd", "tau", "f_ext", "a_des", "v_des")}
    d["active"] = None if I["active"] is None else laid_out(dev(torch, I["active"][:B], torch.int32), layout)
    return d


def call_constrained(hm, D, I, layout, out, compliance=0.0, gravity=GRAVITY, bases="own"):
    return hm.aba_constrained(D["q"], D["qd"], D["tau"], I["targets"], I["rows"], I["poses"], D["active"], D["a_des"], compliance, gravity, D["f_ext"],
                              layout, out=out, bases=I["bases"] if bases == "own" else bases)


def call_impulse(hm, D, I, layout, out, compliance=0.0, bases="own"):
    return hm.constraint_impulse(D["q"], D["qd"], I["targets"], I["rows"], I["poses"], D["active"], D["v_des"], compliance, layout, out=out,
                                 bases=I["bases"] if bases == "own" else bases)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name", list(CASES))
def test_matches_checker(torch_cuda, name, layout, dtype_name):
    torch = torch_cuda
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R, RI = references(name, dtype_name)
    sys_, desc, om = model_of(name)
    hm, km = hip_model(desc), kc.KinModel(desc)
    K, n = len(I["targets"]), desc.n_joints
    for B in BATCHES:
        label = f"{name} B={B} layout={layout} {dtype_name}"
        D = device_inputs(torch, I, B, layout, dtype)
        act = I["active"][:B]
        # ---- accelerations
        qdd, qdd_rows, qdd_guard = outputs(torch, B, (desc.nv,), layout, dtype)
        lam, lam_rows, lam_guard = outputs(torch, B, (K, 6), layout, dtype)
        call_constrained(hm, D, I, layout, (qdd, lam))
        torch.cuda.synchronize()
        assert torch.isnan(qdd_guard).all() and torch.isnan(lam_guard).all(), label + ": wrote past the end"
        x, l = qdd_rows.cpu().numpy().astype(np.float64), lam_rows.cpu().numpy().astype(np.float64).reshape(B, K, 6)
        assert not np.isnan(x).any() and not np.isnan(l).any(), label + ": entries left unwritten"
        check_exact_zeros(l, I, B, label)
        print(f"{label}: cond_inf(KKT) <= {R['cond_kkt'][:B].max():.2e}")
        close_aba(np.concatenate([x, l.reshape(B, -1)], axis=1), np.concatenate([R["qdd"][:B], R["lam"][:B].reshape(B, -1)], axis=1), None, n, u,
                  label=label + " (qdd, lambda)", conds=R["cond_kkt"][:B])
        sub = {k: R[k][:B] for k in ("J", "c")}
        res = rc.constraint_residual(sub, I["rows"], act, x, l, I["a_des"][:B], 0.0)
        scale = np.maximum(1.0, (np.einsum("bij,bj->bi", np.abs(sub["J"]), np.abs(x)) + np.abs(sub["c"]) + np.abs(I["a_des"][:B].reshape(B, -1))).max(axis=1))
        hold_residual(res, scale, R["cond_H"][:B], n, u, label + " constraint equation")
        f = rc.wrenches_on_bodies(km, I["q"][:B], I["targets"], I["bases"], I["poses"], l, I["f_ext"][:B])
        back = om.rnea(I["q"][:B], I["qd"][:B], x, GRAVITY, f) - I["tau"][:B]
        JTl = np.einsum("bji,bj->bi", R["J"][:B], l.reshape(B, -1))
        scale = np.abs(I["tau"][:B]).max(axis=1) + np.abs(R["h"][:B]).max(axis=1) + np.abs(JTl).max(axis=1)
        hold_residual(np.abs(back).max(axis=1), scale, R["cond_H"][:B], n, u, label + " equation of motion")
        # ---- velocities
        qdn, qdn_rows, qdn_guard = outputs(torch, B, (desc.nv,), layout, dtype)
        imp, imp_rows, imp_guard = outputs(torch, B, (K, 6), layout, dtype)
        call_impulse(hm, D, I, layout, (qdn, imp))
        torch.cuda.synchronize()
        assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all(), label + ": impulse wrote past the end"
        v, p = qdn_rows.cpu().numpy().astype(np.float64), imp_rows.cpu().numpy().astype(np.float64).reshape(B, K, 6)
        assert not np.isnan(v).any() and not np.isnan(p).any(), label + ": impulse entries left unwritten"
        check_exact_zeros(p, I, B, label + " impulse")
        close_aba(np.concatenate([v, p.reshape(B, -1)], axis=1), np.concatenate([RI["qd_next"][:B], RI["impulse"][:B].reshape(B, -1)], axis=1), None, n,
                  u, label=label + " (qd+, impulse)", conds=RI["cond_kkt"][:B])
        res = rc.constraint_residual({"J": RI["J"][:B]}, I["rows"], act, v, p, I["v_des"][:B], 0.0)
        scale = np.maximum(1.0, (np.einsum("bij,bj->bi", np.abs(RI["J"][:B]), np.abs(v)) + np.abs(I["v_des"][:B].reshape(B, -1))).max(axis=1))
        hold_residual(res, scale, RI["cond_H"][:B], n, u, label + " velocity constraint")
        H, JTp = RI["H"][:B], np.einsum("bji,bj->bi", RI["J"][:B], p.reshape(B, -1))
        Hv, Hq = np.einsum("bij,bj->bi", H, v), np.einsum("bij,bj->bi", H, I["qd"][:B])
        scale = np.abs(Hv).max(axis=1) + np.abs(Hq).max(axis=1) + np.abs(JTp).max(axis=1)
        hold_residual(np.abs(Hv - Hq - JTp).max(axis=1), scale, RI["cond_H"][:B], n, u, label + " momentum balance")


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name,holes,relist", [("humanoid_mixed", 0, False), ("humanoid_mixed", 0, True), ("humanoid_mixed", 2, False)])
def test_scattered_index_maps(torch_cuda, name, holes, relist, layout, dtype_name):
    """The between-bodies forms on the humanoid with maps that send every DoF and every configuration entry somewhere else (also with two
    indices of each space owned by no joint, holding 7.0 in every state input, and with its joints re-listed, the target and base lists
    translated and the external wrenches in the new order), with test_matches_checker's lists, poses and inputs, against ITS references -- the checker on
    the identity description -- under its bound: close_aba on (qdd, lambda) resp. (qd+, impulse) with cond_inf(KKT).  Guard rows stay
    poisoned; read without moving them back qdd and qd+ miss the reference by more than 1e-3."""
    torch = torch_cuda
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R, RI = references(name, dtype_name)
    sys_, desc, om = model_of(name)
    d, pv, pq, targets, bases, order = scattered_description(name, desc, holes, relist, I["targets"], I["bases"])
    hm = hip_model(d)
    assert relist or hm.kernel_variant.startswith("topo:"), hm.kernel_variant
    B, K, n, nv = 70, len(targets), desc.n_joints, d.nv
    D, J = moved_inputs(torch, I, B, pv, pq, d, order, layout, dtype), dict(I, targets=targets, bases=bases)
    label = f"scattered {name} holes={holes} relist={relist} layout={layout} {dtype_name}"
    for call, ref, x_key, l_key in ((call_constrained, R, "qdd", "lam"), (call_impulse, RI, "qd_next", "impulse")):
        x, x_rows, x_guard = outputs(torch, B, (nv,), layout, dtype)
        lam, lam_rows, lam_guard = outputs(torch, B, (K, 6), layout, dtype)
        call(hm, D, J, layout, (x, lam))
        torch.cuda.synchronize()
        assert torch.isnan(x_guard).all() and torch.isnan(lam_guard).all(), f"{label} {x_key}: wrote past the end"
        raw, l = x_rows.cpu().numpy().astype(np.float64), lam_rows.cpu().numpy().astype(np.float64).reshape(B, K, 6)
        back, free = hp.from_v(raw, pv)
        assert not np.isnan(back).any() and not np.isnan(l).any(), f"{label} {x_key}: entries left unwritten"
        assert x_key == "qdd" or np.all(free == hp.UNOWNED), f"{label}: entries of qd_out no joint owns do not hold those of qd"
        check_exact_zeros(l, I, B, f"{label} {l_key}")
        close_aba(np.concatenate([back, l.reshape(B, -1)], axis=1), np.concatenate([ref[x_key][:B], ref[l_key][:B].reshape(B, -1)], axis=1), None, n, u,
                  label=f"{label} ({x_key}, {l_key})", conds=ref["cond_kkt"][:B])
        hp.assert_misses(hp.keep_order(raw, pv), ref[x_key][:B], f"{label} {x_key}")


def test_parallelogram_known_answer(torch_cuda):
    """The closed-form crank acceleration of the parallelogram linkage: fp64 to 1e-10, fp32 to the forward bound with the KKT matrix's
    conditioning.  AoS and SoA."""
    torch = torch_cuda
    _, desc = parallelogram()
    hm = hip_model(desc)
    q, qd, tau, want = parallelogram_state()
    R = rc.aba_constrained(OracleModel(desc), desc, q, qd, tau, P_TARGETS, P_BASES, P_ROWS, P_POSES, None, None, 0.0, P_GRAVITY)
    B = q.shape[0]
    for layout in (AOS, SOA):
        for dtype in (torch.float64, torch.float32):
            args = [laid_out(dev(torch, x, dtype), layout) for x in (q, qd, tau)]
            qdd, lam = hm.aba_constrained(*args, P_TARGETS, P_ROWS, P_POSES, gravity=P_GRAVITY, layout=layout, bases=P_BASES)
            torch.cuda.synchronize()
            x = (qdd if layout == AOS else qdd.t()).cpu().numpy().astype(np.float64)
            l = (lam.reshape(B, -1) if layout == AOS else lam.t()).cpu().numpy().astype(np.float64)
            assert not l[:, [0, 1, 2, 5]].any() and np.abs(l).max() > 0.1
            if dtype == torch.float64:
                close(x, want, 1.0e-10, label=f"parallelogram fp64 layout={layout}")
            else:
                close_aba(x, want, None, desc.n_joints, U32, label=f"parallelogram fp32 layout={layout}", conds=R["cond_kkt"])


def _raw_between(hm, torch, lib, D, I, layout, dtype, velocity, bases):
    """The _between_ entry point through ctypes (base_joints may be NULL): (first output, wrench output)"""
    sfx = "f64" if dtype == torch.float64 else "f32"
    B = D["q"].shape[0] if layout == AOS else D["q"].shape[1]
    K, nv = len(I["targets"]), I["desc"].nv
    first = torch.empty((B, nv) if layout == AOS else (nv, B), dtype=dtype, device="cuda")
    lam = torch.empty((B, K, 6) if layout == AOS else (6 * K, B), dtype=dtype, device="cuda")
    tgt, rows = np.array(I["targets"], dtype=np.int32), np.array(I["rows"], dtype=np.int32)
    base = None if bases is None else np.array(bases, dtype=np.int32)
    poses = np.ascontiguousarray(I["poses"], dtype=np.float64)
    tail = (K, tgt.ctypes.data, None if base is None else base.ctypes.data, poses.ctypes.data, rows.ctypes.data, D["active"].data_ptr())
    if velocity:
        opts = hm._options(layout, stream=torch.cuda.current_stream().cuda_stream)
        st = getattr(lib, "mh_constraint_impulse_between_" + sfx)(hm._h, B, D["q"].data_ptr(), D["qd"].data_ptr(), *tail, D["v_des"].data_ptr(), 0.0,
                                                                  ctypes.byref(opts), first.data_ptr(), lam.data_ptr())
    else:
        g, ra = hm._root(GRAVITY)
        opts = hm._options(layout, True, True, torch.cuda.current_stream().cuda_stream, root_acceleration=ra)
        st = getattr(lib, "mh_aba_constrained_between_" + sfx)(hm._h, B, D["q"].data_ptr(), D["qd"].data_ptr(), D["tau"].data_ptr(), g,
                                                               D["f_ext"].data_ptr(), *tail, D["a_des"].data_ptr(), 0.0, ctypes.byref(opts),
                                                               first.data_ptr(), lam.data_ptr())
    assert st == 0, lib.mh_last_error()
    torch.cuda.synchronize()
    return first, lam


def test_root_bases_give_the_bits_of_the_rooted_calls(torch_cuda):
    """base_joints = NULL and all -1: both outputs of both entry points equal those of mh_aba_constrained_* / mh_constraint_impulse_*."""
    from mecano_amd import _lib
    torch = torch_cuda
    name = "humanoid_mixed"
    sys_, desc, om = model_of(name)
    hm, B, lib = hip_model(desc), 130, _lib.load()
    I = make_inputs(name, B, seed=2)
    K = len(I["targets"])
    for dtype in (torch.float64, torch.float32):
        for layout in (AOS, SOA):
            D = device_inputs(torch, I, B, layout, dtype)
            want = list(call_constrained(hm, D, I, layout, None, bases=None)) + list(call_impulse(hm, D, I, layout, None, bases=None))
            torch.cuda.synchronize()
            assert not any(torch.isnan(t).any() for t in want)
            for bases in (None, [-1] * K):
                got = list(_raw_between(hm, torch, lib, D, I, layout, dtype, False, bases)) + list(_raw_between(hm, torch, lib, D, I, layout, dtype, True, bases))
                for g, w in zip(got, want):
                    assert torch.equal(g, w), f"layout={layout} {dtype} bases={bases}"
            if layout == AOS:  # the engine's keyword with a list of -1 takes the new entry points as well
                got = list(call_constrained(hm, D, I, layout, None, bases=[-1] * K)) + list(call_impulse(hm, D, I, layout, None, bases=[-1] * K))
                torch.cuda.synchronize()
                assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_nothing_active_gives_the_bits_of_the_free_forward_dynamics(torch_cuda):
    torch = torch_cuda
    name = "humanoid_mixed"
    sys_, desc, om = model_of(name)
    hm, B = hip_model(desc), 70
    I = make_inputs(name, B, seed=2)
    I["active"] = np.zeros_like(I["active"])
    for layout in (AOS, SOA):
        D = device_inputs(torch, I, B, layout, torch.float64)
        qdd, lam = call_constrained(hm, D, I, layout, None)
        free = hm.aba(D["q"], D["qd"], D["tau"], GRAVITY, D["f_ext"], layout)
        qdn, imp = call_impulse(hm, D, I, layout, None)
        torch.cuda.synchronize()
        assert not lam.any() and not imp.any()
        assert torch.equal(qdd, free), f"layout={layout}"
        v = (qdn if layout == AOS else qdn.t()).cpu().numpy()
        close_aba(v, I["qd"], om.crba(I["q"]), desc.n_joints, label=f"nothing active, impulse layout={layout}")


def test_a_nan_state_stays_in_its_own_configuration(torch_cuda):
    torch = torch_cuda
    name = "humanoid_feet_hands"
    sys_, desc, om = model_of(name)
    hm, B, bad = hip_model(desc), 130, 77
    I = make_inputs(name, B, seed=5)
    I["active"][bad] = 0x3F
    for dtype in (torch.float64, torch.float32):
        for layout in (AOS, SOA):
            D = device_inputs(torch, I, B, layout, dtype)
            good = [t.clone() for t in call_constrained(hm, D, I, layout, None)] + [t.clone() for t in call_impulse(hm, D, I, layout, None)]
            Dq = D["q"].clone()
            (Dq if layout == AOS else Dq.t())[bad, :] = float("nan")
            D["q"] = Dq
            got = list(call_constrained(hm, D, I, layout, None)) + list(call_impulse(hm, D, I, layout, None))
            torch.cuda.synchronize()
            for g, w in zip(got, good):
                g, w = (g.reshape(B, -1), w.reshape(B, -1)) if layout == AOS else (g.t(), w.t())
                assert torch.isnan(g[bad]).all(), f"layout={layout} {dtype}: the NaN configuration has numbers in its outputs"
                keep = torch.arange(B, device="cuda") != bad
                assert not torch.isnan(w).any()
                assert torch.equal(g[keep], w[keep]), f"layout={layout} {dtype}: a neighbour of the NaN configuration changed"


_COVER = {}


def cover_reference(torch):
    """The row-cover batch of the first humanoid case: (B, DistinctRows, covered rows, checker results), once for both layouts"""
    if not _COVER:
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        sys_, desc, om = model_of("humanoid_mixed")
        _, targets, bases, masks = CASES["humanoid_mixed"]
        B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
        rows = DistinctRows(sys_, 256, seed=31)
        idx = group_cover(B, grid)
        q, qd, _, tau = rows.rows(idx)
        poses = kc.random_poses(np.random.default_rng(35), len(targets))
        R = rc.aba_constrained(om, desc, q, qd, tau, targets, bases, masks, poses, None, None, 0.0, GRAVITY)
        RI = rc.constraint_impulse(om, desc, q, qd, targets, bases, masks, poses, terms=R)
        _COVER.update(B=B, rows=rows, idx=idx, targets=targets, bases=bases, masks=masks, poses=poses, R=R, RI=RI, desc=desc)
    return _COVER


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the constraint kernel's grid holds (8 per CU), plus a ragged last group: every lane loops over several
    groups of 64.  B distinct rows, poisoned outputs with guard rows, every row group checked, every entry written."""
    torch = torch_cuda
    C = cover_reference(torch)
    desc, B, idx = C["desc"], C["B"], C["idx"]
    hm = hip_model(desc)
    K = len(C["targets"])
    q, qd, _, tau = C["rows"].device(torch, B)
    q, qd, tau = laid_out(q, layout), laid_out(qd, layout), laid_out(tau, layout)
    tol = f32_aba_forward_factor(desc.n_joints) * U64
    for what, R, keys in (("acceleration", C["R"], ("qdd", "lam")), ("impulse", C["RI"], ("qd_next", "impulse"))):
        first, first_rows, first_guard = outputs(torch, B, (desc.nv,), layout, torch.float64)
        lam, lam_rows, lam_guard = outputs(torch, B, (K, 6), layout, torch.float64)
        if what == "acceleration":
            hm.aba_constrained(q, qd, tau, C["targets"], C["masks"], C["poses"], gravity=GRAVITY, layout=layout, out=(first, lam), bases=C["bases"])
        else:
            hm.constraint_impulse(q, qd, C["targets"], C["masks"], C["poses"], layout=layout, out=(first, lam), bases=C["bases"])
        torch.cuda.synchronize()
        cond = float(R["cond_kkt"].max())
        check_cover(first_rows, first_guard, idx, R[keys[0]], tol * cond, label=f"{what} layout={layout}")
        check_cover(lam_rows, lam_guard, idx, R[keys[1]].reshape(len(idx), -1), tol * cond, label=f"{what} wrench layout={layout}")
        del first, lam, first_rows, lam_rows


def test_capture_replay_and_two_contexts(torch_cuda):
    """One eager call per context (it grows the scratch), then both entry points captured in a graph replay to the bits of the eager
    calls; two contexts on two streams at once give the bits of the default context."""
    torch = torch_cuda
    name = "humanoid_mixed"
    sys_, desc, om = model_of(name)
    hm, B = hip_model(desc), 1000
    I = make_inputs(name, B, seed=6)
    D = device_inputs(torch, I, B, AOS, torch.float64)
    ref = [t.clone() for t in call_constrained(hm, D, I, AOS, None)] + [t.clone() for t in call_impulse(hm, D, I, AOS, None)]
    torch.cuda.synchronize()
    views, streams = [hm.context(), hm.context()], [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[torch.zeros_like(t) for t in ref] for _ in views]
    for view in views:
        view.reserve(B)
    for view, s, o in zip(views, streams, outs):  # both in flight before either is waited for
        with torch.cuda.stream(s):
            call_constrained(view, D, I, AOS, (o[0], o[1]))
            call_impulse(view, D, I, AOS, (o[2], o[3]))
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
            call_constrained(view, D, I, AOS, (o[0], o[1]))
            call_impulse(view, D, I, AOS, (o[2], o[3]))
    torch.cuda.synchronize()
    assert not any(t.any() for t in o)  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(o, ref):
        assert torch.equal(got, want)
    for view in views:
        view.close()


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from mecano_amd import _lib
    from test_constrained_dynamics_cpu import model_of as rooted_model_of
    torch = torch_cuda
    sys_, desc, om = rooted_model_of("arm7_weld")
    hm, B, K = hip_model(desc), 10, 2
    lib = _lib.load()
    rng = np.random.default_rng(9)
    q, qd, tau = (dev(torch, rng.uniform(-1.0, 1.0, (B, n))) for n in (desc.nq, desc.nv, desc.nv))
    f = dev(torch, rng.uniform(-2.0, 2.0, (B, desc.n_joints, 6)))
    a = dev(torch, np.zeros((B, K, 6)))
    act = torch.full((B, K), 0x3F, device="cuda", dtype=torch.int32)
    qdd, qdd_guard = poisoned(torch, B, (desc.nv,), torch.float64)
    lam, lam_guard = poisoned(torch, B, (K, 6), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    g = (ctypes.c_double * 3)(*GRAVITY)
    arr = lambda *v: np.array(v, dtype=np.int32)
    tgt, base, rows = arr(2, 6), arr(-1, 2), arr(0b001000, rc.POINT)  # 1 + 3 rows: the arm has 7 DoFs
    ident = np.tile(kc.IDENTITY12, (K, 1))
    skewed = ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    keep = [arr(2, -1), arr(-1, 6), arr(-1, 7), arr(-2, 2), arr(2, 7), arr(-1, 2), arr(rc.POINT, 0x40), arr(0, 0)]

    def untouched(what):
        assert lib.mh_last_error(), what
        for t in (qdd, qdd_guard, lam, lam_guard):
            assert torch.isnan(t).all(), what

    def acc(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), tau=tau.data_ptr(), g=g, f=f.data_ptr(), n=K, t=tgt.ctypes.data, b=base.ctypes.data, p=None,
            r=rows.ctypes.data, act=act.data_ptr(), a=a.data_ptr(), eps=0.0, out=qdd.data_ptr(), lam=lam.data_ptr()):
        st = fn(hm._h, B, q, qd, tau, g, f, n, t, b, p, r, act, a, eps, ctypes.byref(opts), out, lam)
        torch.cuda.synchronize()
        return st

    def imp(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), n=K, t=tgt.ctypes.data, b=base.ctypes.data, p=None, r=rows.ctypes.data, act=act.data_ptr(),
            a=a.data_ptr(), eps=0.0, out=qdd.data_ptr(), lam=lam.data_ptr(), **ignored):
        st = fn(hm._h, B, q, qd, n, t, b, p, r, act, a, eps, ctypes.byref(opts), out, lam)
        torch.cuda.synchronize()
        return st

    shared = {"base = target (first)": dict(b=keep[0].ctypes.data), "base = target (second)": dict(b=keep[1].ctypes.data),
              "base beyond the last joint": dict(b=keep[2].ctypes.data), "base below -1": dict(b=keep[3].ctypes.data),
              "NULL q": dict(q=None), "NULL qd": dict(qd=None), "NULL output": dict(out=None), "NULL target_joints": dict(t=None),
              "NULL target_rows": dict(r=None), "no targets": dict(n=0), "too many targets": dict(n=9),
              "joint out of range": dict(t=keep[4].ctypes.data), "the root body as a target": dict(t=keep[5].ctypes.data, b=None),
              "a mask with bit 6": dict(r=keep[6].ctypes.data), "no bit set": dict(r=keep[7].ctypes.data),
              "negative compliance": dict(eps=-1.0e-9), "NaN compliance": dict(eps=float("nan")), "pose not orthonormal": dict(p=skewed.ctypes.data),
              "output is q": dict(out=q.data_ptr()), "wrench output overlaps the desired motion": dict(lam=a.data_ptr()),
              "outputs overlap": dict(lam=qdd.data_ptr() + 16), "output overlaps active": dict(out=act.data_ptr())}
    only_acc = {"NULL tau": dict(tau=None), "NULL gravity without a root acceleration": dict(g=None), "output is tau": dict(out=tau.data_ptr()),
                "wrench output overlaps f_ext": dict(lam=f.data_ptr())}
    for sfx in ("f64", "f32"):
        for what, kw in {**shared, **only_acc}.items():
            assert acc(getattr(lib, "mh_aba_constrained_between_" + sfx), **kw) == INVALID, what
            untouched(what)
        for what, kw in shared.items():
            assert imp(getattr(lib, "mh_constraint_impulse_between_" + sfx), **kw) == INVALID, what
            untouched(what)
    before = [t.clone() for t in (q, qd, tau)]
    assert acc(lib.mh_aba_constrained_between_f64, B=0) == 0
    assert acc(lib.mh_aba_constrained_between_f64, B=0, q=None, qd=None, tau=None, out=None, lam=None) == 0
    assert imp(lib.mh_constraint_impulse_between_f64, B=0) == 0
    untouched("B = 0")
    assert acc(lib.mh_aba_constrained_between_f64, p=ident.ctypes.data) == 0
    for t, gd in ((qdd, qdd_guard), (lam, lam_guard)):
        assert not torch.isnan(t).any() and torch.isnan(gd).all()
    assert all(torch.equal(x, y) for x, y in zip((q, qd, tau), before))
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_constrained(q, qd, tau, [2, 6], [rc.POINT, rc.WELD], bases=[-1])  # one base for two targets
    with pytest.raises(_lib.MecanoHipError):
        hm.constraint_impulse(q, qd, [2, 6], [0b001000, rc.POINT], bases=[-1, 6])
