"""mh_aba_constrained_* and mh_constraint_impulse_* on the device against the dense KKT checker (tests/constrained_dynamics_check.py, pinned
by tests/test_constrained_dynamics_cpu.py), through the C-ABI (HipModel.aba_constrained / constraint_impulse are the ctypes calls).  Every
output is poisoned and has a guard row behind it: entries left unwritten and writes past the end show.

The bound is helpers.close_aba applied to the matrix actually solved: per configuration
    |x - ref|_inf <= f32_aba_forward_factor(n_joints) cond_inf(KKT of the reference) u max(1, |ref|_inf),   x = (qdd, lambda),
u = 2^-53 or 2^-24; fp32 is held against the fp64 checker on the fp32-rounded inputs.  Because that bound is loose where the KKT matrix is
badly conditioned, two residuals of the device outputs are held beside it with cond_inf(H) in its place: the constraint equation through the
checker's J and c, relative to the sum of the magnitudes of its terms, and the equation of motion through the oracle's inverse dynamics,
relative to |tau| + |h| + |J^T lambda|."""
import ctypes

import numpy as np
import pytest

import constrained_dynamics_check as cc
import helpers as hp
import kinematics_check as kc
from helpers import DistinctRows, U32, check_cover, close_aba, f32_aba_forward_factor, group_cover, poisoned, record_parity
from test_constrained_dynamics_cpu import CASES, GRAVITY, duplicate_compliance, make_inputs, model_of, reference, reference_impulse

pytestmark = pytest.mark.gpu

AOS, SOA = 0, 1
INVALID = 1  # MH_ERR_INVALID_ARGUMENT
B_MAX = 257
BATCHES = (1, 63, 64, 65, 257)  # one ragged wave, one full, one more than full, several
U64 = 2.0 ** -53


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def hip_model(desc):
    from mecano_amd.engine import HipModel
    return HipModel(desc)


def outputs(torch, B, row_shape, layout, dtype):
    """(tensor to pass in out=, its [B, ...] view, guard)"""
    if layout == AOS:
        out, guard = poisoned(torch, B, row_shape, dtype)
        return out, out, guard
    out, guard = poisoned(torch, int(np.prod(row_shape)), (B,), dtype)
    return out, out.t(), guard


def laid_out(x, layout):
    """[B, ...] -> the call's layout: AoS as it is, SoA [entries, B]"""
    return x if layout == AOS else x.reshape(x.shape[0], -1).t().contiguous()


_REFS = {}


def references(name, dtype_name):
    """(inputs, checker result of the accelerations, of the impulse) of B_MAX configurations, once per (case, precision); a smaller batch
    takes the first rows.  fp32: the checker runs in fp64 on the fp32-rounded inputs."""
    key = (name, dtype_name)
    if key not in _REFS:
        I = make_inputs(name, B_MAX, dtype=np.float64 if dtype_name == "f64" else np.float32)
        _REFS[key] = (I, reference(name, I), reference_impulse(name, I))
    return _REFS[key]


def device_inputs(torch, I, B, layout, dtype):
    d = {k: laid_out(dev(torch, I[k][:B], dtype), layout) for k in ("q", "qd", "tau", "f_ext", "a_des", "v_des")}
    d["active"] = None if I["active"] is None else laid_out(dev(torch, I["active"][:B], torch.int32), layout)
    return d


def call_constrained(hm, D, I, layout, out, compliance=0.0, gravity=GRAVITY):
    return hm.aba_constrained(D["q"], D["qd"], D["tau"], I["targets"], I["rows"], I["poses"], D["active"], D["a_des"], compliance, gravity, D["f_ext"],
                              layout, out=out)


def call_impulse(hm, D, I, layout, out, compliance=0.0):
    return hm.constraint_impulse(D["q"], D["qd"], I["targets"], I["rows"], I["poses"], D["active"], D["v_des"], compliance, layout, out=out)


def hold_residual(res, scale, cond_H, n_joints, u, label):
    """res / scale per configuration against f32_aba_forward_factor(n) cond_inf(H) u; logged as achieved / bound like close_aba's"""
    ratio = float((res / (np.maximum(scale, 1.0e-300) * cond_H * u)).max())
    factor = f32_aba_forward_factor(n_joints)
    record_parity(ratio, factor, label)
    assert ratio <= factor, f"{label}: residual / (cond_inf(H) u scale) = {ratio:.3e} > {factor:.3e}"


def check_exact_zeros(lam, I, B, label):
    """rows that are unconstrained or inactive hold exactly 0.0"""
    K = len(I["targets"])
    flat = lam.reshape(B, 6 * K)
    for r in range(B):
        on = np.zeros(6 * K, dtype=bool)
        on[cc.selected_rows(I["rows"], None if I["active"] is None else I["active"][r])] = True
        assert not flat[r][~on].any(), f"{label}: row {r} has a nonzero entry in a row that takes no part"


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name", list(CASES))
def test_matches_checker(torch_cuda, name, layout, dtype_name):
    torch = torch_cuda
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R, RI = references(name, dtype_name)
    sys_, desc, om = model_of(name)
    hm = hip_model(desc)
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
        close_aba(np.concatenate([x, l.reshape(B, -1)], axis=1), np.concatenate([R["qdd"][:B], R["lam"][:B].reshape(B, -1)], axis=1), None, n, u,
                  label=label + " (qdd, lambda)", conds=R["cond_kkt"][:B])
        sub = {k: R[k][:B] for k in ("J", "c")}
        res = cc.constraint_residual(sub, I["rows"], act, x, l, I["a_des"][:B], 0.0)
        scale = np.maximum(1.0, (np.einsum("bij,bj->bi", np.abs(sub["J"]), np.abs(x)) + np.abs(sub["c"]) + np.abs(I["a_des"][:B].reshape(B, -1))).max(axis=1))
        hold_residual(res, scale, R["cond_H"][:B], n, u, label + " constraint equation")
        f = cc.wrenches_on_bodies(desc, I["targets"], I["poses"], l, I["f_ext"][:B])
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
        res = cc.constraint_residual({"J": RI["J"][:B]}, I["rows"], act, v, p, I["v_des"][:B], 0.0)
        scale = np.maximum(1.0, (np.einsum("bij,bj->bi", np.abs(RI["J"][:B]), np.abs(v)) + np.abs(I["v_des"][:B].reshape(B, -1))).max(axis=1))
        hold_residual(res, scale, RI["cond_H"][:B], n, u, label + " velocity constraint")
        H, JTp = RI["H"][:B], np.einsum("bji,bj->bi", RI["J"][:B], p.reshape(B, -1))
        Hv, Hq = np.einsum("bij,bj->bi", H, v), np.einsum("bij,bj->bi", H, I["qd"][:B])
        scale = np.abs(Hv).max(axis=1) + np.abs(Hq).max(axis=1) + np.abs(JTp).max(axis=1)
        hold_residual(np.abs(Hv - Hq - JTp).max(axis=1), scale, RI["cond_H"][:B], n, u, label + " momentum balance")


SCATTERED = [("humanoid30", 0, False), ("humanoid30", 0, True), ("humanoid30", 2, False)]  # (case, holes, joints re-listed)


def scattered_description(name, desc, holes, relist, targets, bases=None):
    """(description on scattered maps, perm_v, perm_q, targets, bases in its listing, order): test_matches_checker's model, targets and rows,
    with every DoF and configuration entry sent somewhere else; relist: its joints listed in a random order, parents possibly after
    children.  The unowned-index case of the constraint, contact and joint-limit tests is taken on this humanoid and not on the mixed tree
    of helpers.mixed_tree, so that the family's own targets, rows, poses, inputs and cached references serve unchanged (its code object
    then runs with dense_maps off).  The two flags asserted below are what rules the identity plans out: kernel_variant, which the callers
    assert too, names the code object and reads the same on any maps, and a re-listed description is asked for no variant."""
    import zlib
    assert hp.maps_flags(desc) == (1, 1)
    rng = np.random.default_rng(zlib.crc32(f"scattered {name} {holes} {relist}".encode()))
    d, pv, pq = hp.scattered_maps(desc, rng, holes)
    order = np.arange(desc.n_joints)  # joint k of the description handed out is joint order[k] of `desc`
    if relist:
        d, order = hp.relisted(d, rng)
        assert any(d.parent[k] > k for k in range(d.n_joints))
        inv = np.argsort(order)
        targets = [int(inv[j]) if j >= 0 else -1 for j in targets]
        bases = None if bases is None else [int(inv[j]) if j >= 0 else -1 for j in bases]
    assert hp.maps_flags(d) == (0, int(holes == 0))  # no plan reserved for identity (or dense) maps can be taken
    return d, pv, pq, targets, bases, order


def moved_inputs(torch, I, B, pv, pq, d, order, layout, dtype, keys=("q", "qd", "tau", "f_ext", "a_des", "v_des")):
    """device_inputs on the scattered description: q through the configuration map, qd and tau through the DoF map, the external wrenches
    in the listing order of its joints, the rest as it is"""
    moved = dict(I)
    if "f_ext" in I:
        moved["f_ext"] = I["f_ext"][:, order]
    moved["q"] = hp.to_q(I["q"][:B], pq, d.nq)
    for k in ("qd", "tau"):
        if k in I:
            moved[k] = hp.to_v(I[k][:B], pv, d.nv)
    D = {k: laid_out(dev(torch, moved[k][:B], dtype), layout) for k in keys if k in moved}
    D["active"] = None if I.get("active") is None else laid_out(dev(torch, I["active"][:B], torch.int32), layout)
    return D


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name,holes,relist", SCATTERED)
def test_scattered_index_maps(torch_cuda, name, holes, relist, layout, dtype_name):
    """aba_constrained and constraint_impulse on the humanoid with maps that send every DoF and every configuration entry somewhere else (also
    with two indices of each space owned by no joint, holding 7.0 in every state input, and with its joints re-listed, the target list
    translated and the external wrenches in the new order), with test_matches_checker's targets, rows, poses and inputs, against ITS references -- the checker on the identity
    description -- under its bound: close_aba on (qdd, lambda) resp. (qd+, impulse) with cond_inf(KKT).  The state goes in through the
    maps, qdd and qd+ come back through the DoF map, multipliers and impulses do not move.  Guard rows stay poisoned; read without moving
    them back qdd and qd+ miss the reference by more than 1e-3."""
    torch = torch_cuda
    dtype, u = (torch.float64, U64) if dtype_name == "f64" else (torch.float32, U32)
    I, R, RI = references(name, dtype_name)
    sys_, desc, om = model_of(name)
    d, pv, pq, targets, _, order = scattered_description(name, desc, holes, relist, I["targets"])
    hm = hip_model(d)
    assert relist or hm.kernel_variant.startswith("topo:"), hm.kernel_variant
    B, K, n, nv = 70, len(targets), desc.n_joints, d.nv
    D, J = moved_inputs(torch, I, B, pv, pq, d, order, layout, dtype), dict(I, targets=targets)
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


def test_nothing_active_is_the_free_forward_dynamics_and_null_arguments_are_zeros(torch_cuda):
    """`active` all zero: lambda exactly zero and qdd that of mh_aba_* to the forward bound; qd unchanged by the impulse.  active = NULL is
    every row active, a_des = NULL is zeros, lambda_out = NULL is allowed."""
    torch = torch_cuda
    name = "humanoid30"
    sys_, desc, om = model_of(name)
    hm, B = hip_model(desc), 70
    I = make_inputs(name, B, seed=2)
    I["active"] = np.zeros_like(I["active"])
    D = device_inputs(torch, I, B, AOS, torch.float64)
    qdd, lam = call_constrained(hm, D, I, AOS, None)
    free = hm.aba(D["q"], D["qd"], D["tau"], GRAVITY, D["f_ext"])
    qdn, imp = call_impulse(hm, D, I, AOS, None)
    torch.cuda.synchronize()
    assert not lam.any() and not imp.any()
    H = om.crba(I["q"])
    close_aba(qdd.cpu().numpy(), om.aba(I["q"], I["qd"], I["tau"], GRAVITY, I["f_ext"]), H, desc.n_joints, label="nothing active")
    close_aba(qdd.cpu().numpy(), free.cpu().numpy(), H, desc.n_joints, label="nothing active against mh_aba")
    close_aba(qdn.cpu().numpy(), I["qd"], H, desc.n_joints, label="nothing active, impulse")
    I["active"], I["a_des"] = None, np.zeros_like(I["a_des"])
    R = reference(name, I)
    D["active"] = D["a_des"] = None
    qdd2, none = call_constrained(hm, D, I, AOS, (torch.empty_like(qdd), None))
    torch.cuda.synchronize()
    assert none is None
    close_aba(qdd2.cpu().numpy(), R["qdd"], None, desc.n_joints, label="NULL active, NULL a_des", conds=R["cond_kkt"])


def test_root_acceleration_is_honoured(torch_cuda):
    torch = torch_cuda
    name = "onedof12"
    sys_, desc, om = model_of(name)
    hm, B = hip_model(desc), 40
    I = make_inputs(name, B, seed=4)
    root = (0.4, -0.3, 0.2, 1.0, -2.0, 9.0)
    R = cc.aba_constrained(om, desc, I["q"], I["qd"], I["tau"], I["targets"], I["rows"], I["poses"], I["active"], I["a_des"], 0.0, root, I["f_ext"])
    for layout in (AOS, SOA):
        D = device_inputs(torch, I, B, layout, torch.float64)
        qdd, lam = call_constrained(hm, D, I, layout, None, gravity=root)
        torch.cuda.synchronize()
        x = (qdd if layout == AOS else qdd.t()).cpu().numpy()
        l = (lam.reshape(B, -1) if layout == AOS else lam.t()).cpu().numpy()
        close_aba(np.concatenate([x, l], axis=1), np.concatenate([R["qdd"], R["lam"].reshape(B, -1)], axis=1), None, desc.n_joints,
                  label=f"root acceleration layout={layout}", conds=R["cond_kkt"])


def test_duplicated_target_splits_lambda_and_halves_the_compliance(torch_cuda):
    torch = torch_cuda
    name = "humanoid30"
    sys_, desc, om = model_of(name)
    eps, cond = duplicate_compliance()
    assert cond < 1.0e4
    hm, B = hip_model(desc), 70
    I = make_inputs(name, B, seed=3, with_active=False)
    pose, a = I["poses"][:1], I["a_des"][:, :1]
    q, qd, tau = (dev(torch, I[k]) for k in ("q", "qd", "tau"))
    f = dev(torch, I["f_ext"])
    qdd2, lam2 = hm.aba_constrained(q, qd, tau, [6, 6], [cc.POINT, cc.POINT], np.tile(pose, (2, 1)), None, dev(torch, np.tile(a, (1, 2, 1))), eps, GRAVITY, f)
    qdd1, lam1 = hm.aba_constrained(q, qd, tau, [6], [cc.POINT], pose, None, dev(torch, a), eps / 2, GRAVITY, f)
    torch.cuda.synchronize()
    two = cc.aba_constrained(om, desc, I["q"], I["qd"], I["tau"], [6, 6], [cc.POINT, cc.POINT], np.tile(pose, (2, 1)), None, np.tile(a, (1, 2, 1)), eps,
                             GRAVITY, I["f_ext"])
    half = 0.5 * lam1.cpu().numpy()[:, 0]
    close_aba(qdd2.cpu().numpy(), qdd1.cpu().numpy(), None, desc.n_joints, label="duplicate: qdd", conds=two["cond_kkt"])
    close_aba(lam2.cpu().numpy()[:, 0], half, None, desc.n_joints, label="duplicate: lambda 0", conds=two["cond_kkt"])
    close_aba(lam2.cpu().numpy()[:, 1], half, None, desc.n_joints, label="duplicate: lambda 1", conds=two["cond_kkt"])
    assert np.abs(half).max() > 0.1


def test_a_singular_row_is_nan_in_its_own_outputs_only(torch_cuda):
    """A pivot that is not positive and finite: every output of that configuration is NaN, its neighbours are untouched.  Made with a NaN
    in the state of one configuration (a singular set of rows meets a pivot of either sign, a rounding away from zero)."""
    torch = torch_cuda
    name = "humanoid30"
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
                assert torch.isnan(g[bad]).all(), f"layout={layout} {dtype}: the singular configuration has numbers in its outputs"
                keep = torch.arange(B, device="cuda") != bad
                assert torch.equal(g[keep], w[keep]), f"layout={layout} {dtype}: a neighbour of the singular configuration changed"


_COVER = {}


def cover_reference(torch):
    """The row-cover batch: (B, grid, DistinctRows, covered rows, inputs of those rows, checker result), once for both layouts"""
    if not _COVER:
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        sys_, desc, om = model_of("humanoid30")
        B, grid = 2 * 8 * cus * 64 + 64 + 37, 8 * cus
        rows = DistinctRows(sys_, 256, seed=31)
        idx = group_cover(B, grid)
        q, qd, _, tau = rows.rows(idx)
        targets, masks, poses = [6, 12], [cc.WELD, cc.WELD], kc.random_poses(np.random.default_rng(35), 2)
        R = cc.aba_constrained(om, desc, q, qd, tau, targets, masks, poses, None, None, 0.0, GRAVITY)
        RI = cc.constraint_impulse(om, desc, q, qd, targets, masks, poses)
        _COVER.update(B=B, rows=rows, idx=idx, targets=targets, masks=masks, poses=poses, R=R, RI=RI, desc=desc)
    return _COVER


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout):
    """More than twice the waves the constraint kernel's grid holds (8 per CU), plus a ragged last group: every lane loops over several
    groups of 64.  B distinct rows, poisoned outputs with guard rows, every row group checked, every entry written.  Both feet welded."""
    torch = torch_cuda
    C = cover_reference(torch)
    desc, B, idx = C["desc"], C["B"], C["idx"]
    hm = hip_model(desc)
    q, qd, _, tau = C["rows"].device(torch, B)
    q, qd, tau = laid_out(q, layout), laid_out(qd, layout), laid_out(tau, layout)
    tol = f32_aba_forward_factor(desc.n_joints) * U64
    for what, R, keys in (("acceleration", C["R"], ("qdd", "lam")), ("impulse", C["RI"], ("qd_next", "impulse"))):
        first, first_rows, first_guard = outputs(torch, B, (desc.nv,), layout, torch.float64)
        lam, lam_rows, lam_guard = outputs(torch, B, (2, 6), layout, torch.float64)
        if what == "acceleration":
            hm.aba_constrained(q, qd, tau, C["targets"], C["masks"], C["poses"], gravity=GRAVITY, layout=layout, out=(first, lam))
        else:
            hm.constraint_impulse(q, qd, C["targets"], C["masks"], C["poses"], layout=layout, out=(first, lam))
        torch.cuda.synchronize()
        cond = float(R["cond_kkt"].max())
        check_cover(first_rows, first_guard, idx, R[keys[0]], tol * cond, label=f"{what} layout={layout}")
        check_cover(lam_rows, lam_guard, idx, R[keys[1]].reshape(len(idx), -1), tol * cond, label=f"{what} wrench layout={layout}")
        del first, lam, first_rows, lam_rows


def test_reserve_capture_replay_and_two_contexts(torch_cuda):
    """reserve(B), one call, then both entry points captured in a graph (they allocate nothing) replay to the bits of the eager calls;
    two contexts on two streams at once give the bits of the default context."""
    torch = torch_cuda
    name = "humanoid30"
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
    torch = torch_cuda
    name = "arm7_weld"
    sys_, desc, om = model_of(name)
    hm, B, K = hip_model(desc), 10, 2
    lib = _lib.load()
    I = make_inputs(name, B)
    q, qd, tau = (dev(torch, I[k]) for k in ("q", "qd", "tau"))
    f = dev(torch, I["f_ext"])
    a = dev(torch, np.zeros((B, K, 6)))
    act = torch.full((B, K), 0x3F, device="cuda", dtype=torch.int32)
    qdd, qdd_guard = poisoned(torch, B, (desc.nv,), torch.float64)
    lam, lam_guard = poisoned(torch, B, (K, 6), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    g = (ctypes.c_double * 3)(*GRAVITY)
    tgt, rows = np.array([2, 6], dtype=np.int32), np.array([0b001000, cc.POINT], dtype=np.int32)  # 1 + 3 rows: the arm has 7 DoFs
    ident = np.tile(kc.IDENTITY12, (K, 1))
    skewed, mirrored = ident.copy(), ident.copy()
    skewed[1, 0] = 1.0 + 1.0e-6
    mirrored[0, 8] = -1.0
    arr = lambda *v: np.array(v, dtype=np.int32)
    keep = [arr(2, 7), arr(-1, 2), arr(cc.POINT, 0x40), arr(-1, cc.WELD), arr(0, 0)]

    def untouched(what):
        assert lib.mh_last_error(), what
        for t in (qdd, qdd_guard, lam, lam_guard):
            assert torch.isnan(t).all(), what

    def acc(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), tau=tau.data_ptr(), g=g, f=f.data_ptr(), n=K, t=tgt.ctypes.data, p=None, r=rows.ctypes.data,
            act=act.data_ptr(), a=a.data_ptr(), eps=0.0, out=qdd.data_ptr(), lam=lam.data_ptr()):
        st = fn(hm._h, B, q, qd, tau, g, f, n, t, p, r, act, a, eps, ctypes.byref(opts), out, lam)
        torch.cuda.synchronize()
        return st

    def imp(fn, B=B, q=q.data_ptr(), qd=qd.data_ptr(), n=K, t=tgt.ctypes.data, p=None, r=rows.ctypes.data, act=act.data_ptr(), a=a.data_ptr(),
            eps=0.0, out=qdd.data_ptr(), lam=lam.data_ptr(), **ignored):
        st = fn(hm._h, B, q, qd, n, t, p, r, act, a, eps, ctypes.byref(opts), out, lam)
        torch.cuda.synchronize()
        return st

    shared = {"NULL q": dict(q=None), "NULL qd": dict(qd=None), "NULL output": dict(out=None), "NULL target_joints": dict(t=None),
              "NULL target_rows": dict(r=None), "no targets": dict(n=0), "too many targets": dict(n=9),
              "joint out of range": dict(t=keep[0].ctypes.data), "the root body": dict(t=keep[1].ctypes.data),
              "a mask with bit 6": dict(r=keep[2].ctypes.data), "a negative mask": dict(r=keep[3].ctypes.data), "no bit set": dict(r=keep[4].ctypes.data),
              "negative compliance": dict(eps=-1.0e-9), "NaN compliance": dict(eps=float("nan")),
              "pose not orthonormal": dict(p=skewed.ctypes.data), "pose a reflection": dict(p=mirrored.ctypes.data),
              "output is q": dict(out=q.data_ptr()), "output is qd": dict(out=qd.data_ptr()), "wrench output overlaps the desired motion": dict(lam=a.data_ptr()),
              "outputs overlap": dict(lam=qdd.data_ptr() + 16), "output overlaps active": dict(out=act.data_ptr())}
    only_acc = {"NULL tau": dict(tau=None), "NULL gravity without a root acceleration": dict(g=None), "output is tau": dict(out=tau.data_ptr()),
                "wrench output overlaps f_ext": dict(lam=f.data_ptr())}
    for sfx in ("f64", "f32"):
        for what, kw in {**shared, **only_acc}.items():
            assert acc(getattr(lib, "mh_aba_constrained_" + sfx), **kw) == INVALID, what
            untouched(what)
        for what, kw in shared.items():
            assert imp(getattr(lib, "mh_constraint_impulse_" + sfx), **kw) == INVALID, what
            untouched(what)
    before = [t.clone() for t in (q, qd, tau)]
    assert acc(lib.mh_aba_constrained_f64, B=0) == 0 and acc(lib.mh_aba_constrained_f64, B=0, q=None, qd=None, tau=None, out=None, lam=None) == 0
    assert imp(lib.mh_constraint_impulse_f64, B=0) == 0
    untouched("B = 0")
    locked = hip_model(desc)
    modes = np.zeros(desc.n_joints, dtype=np.int32)
    modes[3] = 1
    locked.set_joint_source_modes(modes)
    assert lib.mh_aba_constrained_f64(locked._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, None, K, tgt.ctypes.data, None, rows.ctypes.data, None,
                                      None, 0.0, ctypes.byref(opts), qdd.data_ptr(), lam.data_ptr()) == INVALID
    untouched("acceleration-source joints")
    assert acc(lib.mh_aba_constrained_f64, p=ident.ctypes.data) == 0
    for t, gd in ((qdd, qdd_guard), (lam, lam_guard)):
        assert not torch.isnan(t).any() and torch.isnan(gd).all()
    assert all(torch.equal(x, y) for x, y in zip((q, qd, tau), before))
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_constrained(q, qd, tau, [2, 6], [cc.POINT])  # one mask for two targets
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_constrained(q, qd, tau, [2, 6], [cc.POINT, cc.WELD], out=(torch.empty((B, desc.nv + 1), dtype=torch.float64, device="cuda"), None))
    with pytest.raises(ValueError):
        hm.constraint_impulse(q, qd, [2, 6], [cc.POINT, cc.WELD], active=act.to(torch.int64))
