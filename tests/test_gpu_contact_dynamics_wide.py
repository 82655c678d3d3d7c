"""mh_contact_impulse_* on the device where tests/test_gpu_contact_dynamics.py does not reach: every K the two kernel builds take with idle
register slots (3 on the build of 4, 5-7 on the build of 8; fp64 from more than 64 KB of LDS), one friction coefficient per contact, a
stale impulse_init, scaled normals, coefficients beyond the square root of the number range, the optional arguments one at a time, and a
NaN in the velocities.  The comparisons are those of tests/test_contact_dynamics_cpu.py (held_to_kkt, held_to_H), where
test_planted_faults_are_rejected_by_the_comparisons_of_the_device_tests holds each of them to the faults it is here to catch.  Every
output is poisoned and has a guard row behind it."""
import numpy as np
import pytest

import contact_dynamics_check as cd
import constrained_dynamics_check as cc
from helpers import DistinctRows, U32, check_cover, close_aba, f32_aba_forward_factor, group_cover
from test_contact_dynamics_cpu import (B_CPU, FEW_SWEEPS_CASES, MANY_SWEEPS, case_of, held_to_H, held_to_kkt, make_inputs, mixed_mu, model_of, solve,
                                       solve_with_fault, stale_start, wide_inputs)
from test_gpu_constrained_dynamics import AOS, B_MAX, BATCHES, SOA, U64, dev, hip_model, hold_residual, laid_out, torch_cuda  # noqa: F401
from test_gpu_contact_dynamics import device_inputs, set_path, three_outputs
from test_launch_plans_cpu import Planner

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "f32"]
_REFS = {}


def precision(torch, dtype_name):
    """(torch dtype, numpy dtype the inputs are rounded to, unit roundoff)"""
    return (torch.float64, np.float64, U64) if dtype_name == "f64" else (torch.float32, np.float32, U32)


def problem(name, dtype_name, v_normal=True):
    """(inputs, checker terms, conditioning) of B_MAX configurations with random active in {0, 1, -1, 7} and random v_normal, once per
    key; a smaller batch takes the first rows.  fp32: the fp64 checker on the fp32-rounded inputs.  The conditioning -- H, J, cond_inf(H),
    cond_inf of the stick system's KKT matrix -- is that of contact_dynamics_check.contact_impulse, which forms it from the states alone."""
    key = (name, dtype_name)
    if key not in _REFS:
        I = wide_inputs(name, B_MAX, np.float64 if dtype_name == "f64" else np.float32)
        _, desc, om = model_of(name)
        stick = cc.constraint_impulse(om, desc, I["q"], I["qd"], I["targets"], [cc.POINT] * len(I["targets"]), I["poses"], None, None, I["compliance"])
        _REFS[key] = (I, {}, dict(cond_H=stick["cond_H"], cond_kkt=stick["cond_kkt"]))
    I, terms, frame = _REFS[key]
    if v_normal not in terms:
        _, desc, om = model_of(name)
        terms[v_normal] = cd.terms(om, desc, I["q"], I["qd"], I["targets"], I["poses"], I["normals"], I["v_normal"] if v_normal else None)
    return I, terms[v_normal], frame


def reference(name, dtype_name, mu, sweeps, stale=False, active=True, v_normal=True):
    """(inputs, stale start or None, checker result): the checker's sweeps (solve_with_fault without a fault: contact_impulse to the bit,
    test_planted_faults_are_rejected_by_the_comparisons_of_the_device_tests) on the terms formed once per problem"""
    I, T, frame = problem(name, dtype_name, v_normal)
    init = stale_start(I) if stale else None
    R = solve_with_fault(name, I, mu, sweeps, None, I["active"] if active else None, I["v_normal"] if v_normal else None, init, T)
    assert not np.isnan(R["impulse"]).any() and np.abs(R["impulse"]).max() > 0.1
    return I, init, dict(R, H=T["H"], J=T["J"], **frame)


def call(hm, D, I, mu, sweeps, layout, out=None, init=None, active=True, v_normal=True, normals=None):
    return hm.contact_impulse(D["q"], D["qd"], I["targets"], mu, I["poses"], D["normals"] if normals is None else normals, D["active"] if active else None,
                              D["v_normal"] if v_normal else None, I["compliance"], sweeps, init, layout, out)


def run_poisoned(torch, hm, D, I, mu, sweeps, layout, dtype, B, nv, label, init=None, active=True, v_normal=True):
    """the call into poisoned outputs: (qd_out [B, nv], impulse_out [B, K, 6], residual_out [B]) as fp64 arrays, every entry written,
    nothing written behind the end"""
    K = len(I["targets"])
    (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, nv, K, layout, dtype)
    call(hm, D, I, mu, sweeps, layout, (qdn, imp, res), init, active, v_normal)
    torch.cuda.synchronize()
    assert torch.isnan(qdn_guard).all() and torch.isnan(imp_guard).all() and torch.isnan(res_guard).all(), label + ": wrote past the end"
    v, p = qdn_rows.cpu().numpy().astype(np.float64), imp_rows.cpu().numpy().astype(np.float64).reshape(B, K, 6)
    r = res_rows.cpu().numpy().astype(np.float64)
    assert not np.isnan(v).any() and not np.isnan(p).any() and not np.isnan(r).any(), label + ": entries left unwritten"
    return v, p, r


def hold_all(v, p, r, I, R, B, n, u, label, active=True):
    """the assertions of test_gpu_contact_dynamics.test_matches_checker: exact zeros, close_aba with cond_kkt on (qd+, impulse) and on the
    residual, the momentum balance with cond_inf(H)"""
    rows = slice(0, B)
    assert not p[:, :, :3].any(), label + ": an angular row is not exactly zero"
    if active:
        assert not p[I["active"][:B] == 0].any(), label + ": an open contact has an impulse"
    print(f"{label}: |qd+ - ref| = {np.abs(v - R['qd_next'][:B]).max():.3e}, |impulse - ref| = {np.abs(p - R['impulse'][:B]).max():.3e}, "
          f"|residual - ref| = {np.abs(r - R['residual'][:B]).max():.3e}, cond_kkt <= {R['cond_kkt'][:B].max():.2e}")
    held_to_kkt(v, p, R, rows, n, u, label)
    close_aba(r[:, None], R["residual"][:B, None], None, n, u, label=label + " residual", conds=R["cond_kkt"][:B])
    H, JTp = R["H"][:B], np.einsum("bji,bj->bi", R["J"][:B], p.reshape(B, -1))
    Hv, Hq = np.einsum("bij,bj->bi", H, v), np.einsum("bij,bj->bi", H, I["qd"][:B])
    scale = np.abs(Hv).max(axis=1) + np.abs(Hq).max(axis=1) + np.abs(JTp).max(axis=1)
    hold_residual(np.abs(Hv - Hq - JTp).max(axis=1), scale, R["cond_H"][:B], n, u, label + " momentum balance")


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name", list(MANY_SWEEPS))
def test_every_K_with_mixed_mu_matches_checker(torch_cuda, name, layout, dtype_name):
    """K = 3 on the build of 4 contacts, K = 5, 6, 7 on the build of 8: the guards of the idle register slots, ld = 6 K in both index
    functions, and in fp64 69 120, 96 768 and 129 024 bytes of LDS per workgroup."""
    torch = torch_cuda
    dtype, _, u = precision(torch, dtype_name)
    mu = mixed_mu(len(case_of(name)[1]))
    I, _, R = reference(name, dtype_name, mu, MANY_SWEEPS[name])
    _, desc, om = model_of(name)
    hm = hip_model(desc)
    for B in BATCHES:
        label = f"{name} B={B} layout={layout} {dtype_name} mixed mu"
        D = device_inputs(torch, I, B, layout, dtype)
        v, p, r = run_poisoned(torch, hm, D, I, mu, MANY_SWEEPS[name], layout, dtype, B, desc.nv, label)
        hold_all(v, p, r, I, R, B, desc.n_joints, u, label)


@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("name", FEW_SWEEPS_CASES)
def test_few_sweeps_from_a_stale_start_are_held_to_cond_H(torch_cuda, name, layout, dtype_name, sweeps):
    """One and three sweeps from an impulse_init no call returned (outside the cones, nonzero angular rows, nonzero on open contacts), with
    MIXED_MU: impulse_out under close_aba with cond_inf(H) in the place of cond_inf(KKT).  On humanoid30_k8 the latter reaches 9e8 and
    allows a relative error of 6e3 in fp32 -- no fault can fail it -- while after a few sweeps nothing has been amplified beyond a few
    products with S = J H^-1 J^T, whose formation cond(H) conditions.  The bound is not derived rigorously; the same sweeps on S and b
    rounded to fp32 (contact_dynamics_check.contact_impulse with precision=np.float32) stay below 0.001 of it on every case here.
    humanoid30_k8_soft is the case at which this comparison rejects a dropped eps lambda_k."""
    torch = torch_cuda
    dtype, _, u = precision(torch, dtype_name)
    mu = mixed_mu(len(case_of(name)[1]))
    I, init, R = reference(name, dtype_name, mu, sweeps, stale=True)
    _, desc, om = model_of(name)
    hm = hip_model(desc)
    for B in (65, 257):
        label = f"{name} B={B} layout={layout} {dtype_name} {sweeps} sweeps"
        D = device_inputs(torch, I, B, layout, dtype)
        start = laid_out(dev(torch, init[:B], dtype), layout)
        v, p, r = run_poisoned(torch, hm, D, I, mu, sweeps, layout, dtype, B, desc.nv, label, init=start)
        held_to_H(p, R, slice(0, B), desc.n_joints, u, label)
        hold_all(v, p, r, I, R, B, desc.n_joints, u, label)  # (with the exact zeros: angular rows and open contacts, despite the start)


@pytest.mark.parametrize("name,dtype_name", [("humanoid30_k5", "f64"), ("humanoid30_k6", "f64"), ("humanoid30_k7", "f64"), ("humanoid30_k7", "f32"),
                                             ("humanoid30_k3", "f32")])
def test_resident_and_streamed_solves_give_the_same_bits_at_every_K(torch_cuda, name, dtype_name):
    torch = torch_cuda
    dtype, np_dtype, _ = precision(torch, dtype_name)
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 200
    I = wide_inputs(name, B, np_dtype, seed=2)
    mu, init = mixed_mu(len(I["targets"])), stale_start(I)
    try:
        for layout in (AOS, SOA):
            D = device_inputs(torch, I, B, layout, dtype)
            start = laid_out(dev(torch, init, dtype), layout)
            got = []
            for path in (1, 0, -1):
                set_path(hm, path)
                got.append([t.clone() for t in call(hm, D, I, mu, 30, layout, init=start)])
            torch.cuda.synchronize()
            assert got[0][1].any() and not torch.isnan(got[0][0]).any()
            for a, b, c in zip(*got):
                assert torch.equal(a, b) and torch.equal(a, c), f"{name} {dtype_name} layout={layout}: the two paths differ"
    finally:
        set_path(hm, -1)


_COVER = {}


def cover_reference(torch, hip_lib):
    if not _COVER:
        name = "humanoid30_k7"
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        sys_, desc, om = model_of(name)
        resident, lds, per_cu, grid, _ = (int(x) for x in Planner(hip_lib, "arm7").plan("contact_solve", 7, 8, -1, cus, 1 << 20))
        assert (resident, lds, per_cu, grid) == (1, 129024, 1, cus)
        B = 2 * grid * 64 + 64 + 37
        rows = DistinctRows(sys_, 256, seed=43)
        idx = group_cover(B, grid)
        q, qd, _, _ = rows.rows(idx)
        I = make_inputs(name, 1)
        mu = mixed_mu(7)
        R = cd.contact_impulse(om, desc, q, qd, I["targets"], mu, I["poses"], None, None, None, 0.0, 2)
        _COVER.update(B=B, rows=rows, idx=idx, targets=I["targets"], poses=I["poses"], mu=mu, R=R, desc=desc)
    return _COVER


def test_device_filling_batch_with_one_wave_per_cu_covers_every_row_group(torch_cuda, hip_lib):
    """K = 7 in fp64: 129 024 bytes of LDS, one workgroup per CU, the grid the CU count; more than twice the grid's waves plus a ragged
    last group.  B distinct rows, every row group checked, every entry written.  2 sweeps, normals, active and v_normal NULL."""
    torch = torch_cuda
    C = cover_reference(torch, hip_lib)
    desc, B, idx, R = C["desc"], C["B"], C["idx"], C["R"]
    hm = hip_model(desc)
    q, qd, _, _ = C["rows"].device(torch, B)
    (qdn, qdn_rows, qdn_guard), (imp, imp_rows, imp_guard), (res, res_rows, res_guard) = three_outputs(torch, B, desc.nv, 7, AOS, torch.float64)
    hm.contact_impulse(q, qd, C["targets"], C["mu"], C["poses"], iterations=2, layout=AOS, out=(qdn, imp, res))
    torch.cuda.synchronize()
    tol = f32_aba_forward_factor(desc.n_joints) * U64 * float(R["cond_kkt"].max())
    check_cover(qdn_rows, qdn_guard, idx, R["qd_next"], tol, label="qd+ K=7")
    check_cover(imp_rows, imp_guard, idx, R["impulse"].reshape(len(idx), -1), tol, label="impulse K=7")
    check_cover(res_rows, res_guard, idx, R["residual"], tol, label="residual K=7")
    assert np.abs(R["impulse"]).max() > 0.1


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_normals_scaled_by_powers_of_two_give_the_same_bits(torch_cuda, layout, dtype_name):
    """n.n scales by 4^p exactly, its root and the reciprocal by exact powers of two: the unit normal, and with it every output, has the
    bits of the unscaled call.  A kernel that skipped the normalisation differs in every row."""
    torch = torch_cuda
    dtype, np_dtype, _ = precision(torch, dtype_name)
    name = "humanoid30_k5"
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 130
    I = wide_inputs(name, B, np_dtype, seed=3)
    D = device_inputs(torch, I, B, layout, dtype)
    factors = 2.0 ** np.random.default_rng(6).integers(-10, 11, (B, 5, 1))
    assert factors.min() < 0.01 and factors.max() > 100.0
    scaled = laid_out(dev(torch, I["normals"] * factors, dtype), layout)
    want = [t.clone() for t in call(hm, D, I, mixed_mu(5), 30, layout)]
    got = call(hm, D, I, mixed_mu(5), 30, layout, normals=scaled)
    torch.cuda.synchronize()
    assert want[1].any() and not torch.isnan(want[0]).any()
    for g, w, what in zip(got, want, ("qd_out", "impulse_out", "residual_out")):
        assert torch.equal(g, w), f"{what} layout={layout} {dtype_name}: the length of the given normals shows"


_STICK = {}


def stick_rows():
    """(inputs, rows, stick impulses, normals in the target frames) of test_stick_inside_the_cone_is_the_bilateral_solution on humanoid30:
    the configurations whose stick solution lies inside every cone of mu = 100 with a tenth of the opening to spare"""
    if not _STICK:
        name, mu = "humanoid30", 100.0
        I = make_inputs(name, B_CPU)
        _, desc, om = model_of(name)
        K = len(I["targets"])
        stick = cc.constraint_impulse(om, desc, I["q"], I["qd"], I["targets"], [cc.POINT] * K, I["poses"], None, None, I["compliance"])
        n = cd.terms(om, desc, I["q"], I["qd"], I["targets"], I["poses"], I["normals"])["n"]
        ls = stick["impulse"][:, :, 3:]
        sn = np.einsum("bki,bki->bk", n, ls)
        st = np.linalg.norm(ls - sn[:, :, None] * n, axis=2)
        _STICK.update(I=I, inside=((sn > 0) & (st <= 0.9 * mu * sn)).all(axis=1), ls=ls)
    return _STICK["I"], _STICK["inside"], _STICK["ls"]


LARGE_MU = [("f64", 1.0e20), ("f32", 1.0e20), ("f64", 1.0e200)]


@pytest.mark.parametrize("dtype_name,big", LARGE_MU)
def test_a_very_large_mu_is_stick(torch_cuda, dtype_name, big):
    """mu whose square leaves the number range (fp32: from 1.85e19, fp64: from 1.34e154), in every slot and in one slot of MIXED_MU, 30
    sweeps against the checker at the bound of test_every_K_with_mixed_mu_matches_checker; and the impulses of 1000 sweeps with that mu
    against those with mu = 100 at the stick tests' 1e-9 scale on the configurations whose stick solution lies inside the cones of
    mu = 100 (in both precisions: the two calls reach the same bits there).  The projection in the form s' = (s + mu r) / (1 + mu^2)
    returns s' = 0 and the origin at such a mu; contact_project works a cone wider than 45 degrees with 1 / mu."""
    torch = torch_cuda
    dtype, np_dtype, u = precision(torch, dtype_name)
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm = hip_model(desc)
    for mu in ([big] * 4, [0.0, 0.3, big, 0.8]):
        I, _, R = reference(name, dtype_name, mu, 30)
        for layout in (AOS, SOA):
            for B in (65, B_MAX):
                label = f"{name} B={B} layout={layout} {dtype_name} mu={mu}"
                D = device_inputs(torch, I, B, layout, dtype)
                v, p, r = run_poisoned(torch, hm, D, I, mu, 30, layout, dtype, B, desc.nv, label)
                hold_all(v, p, r, I, R, B, desc.n_joints, u, label)
    J, inside, ls = stick_rows()
    assert inside.sum() * 2 >= B_CPU
    D = device_inputs(torch, J, B_CPU, AOS, dtype)
    _, wide, _ = call(hm, D, J, [big] * 4, 1000, AOS, active=False, v_normal=False)
    _, hundred, _ = call(hm, D, J, [100.0] * 4, 1000, AOS, active=False, v_normal=False)
    torch.cuda.synchronize()
    wide, hundred = wide.cpu().numpy().astype(np.float64)[:, :, 3:], hundred.cpu().numpy().astype(np.float64)[:, :, 3:]
    scale = max(1.0, np.abs(ls[inside]).max())
    print(f"{dtype_name} mu={big:g}: |lam - lam(mu = 100)| = {np.abs(wide - hundred)[inside].max():.3e} on {inside.sum()} stick rows, "
          f"|lam - stick| = {np.abs(wide - ls)[inside].max():.3e}, scale {scale:.2f}")
    assert np.abs(hundred[inside]).max() > 0.1
    assert np.abs(wide - hundred)[inside].max() <= 1.0e-9 * scale


def test_a_mu_beyond_the_range_of_fp32_is_refused_there_and_taken_in_fp64(torch_cuda):
    """mu = 1e39 is finite in fp64 and infinite as a float: mh_contact_impulse_f32 refuses it and leaves the outputs untouched (the header's
    list); mh_contact_impulse_f64 takes it like any other."""
    from mecano_amd import _lib
    torch = torch_cuda
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B, K = hip_model(desc), 65, 4
    I = wide_inputs(name, B, np.float32)
    mu = [0.5, 1.0e39, 0.5, 0.5]
    D = device_inputs(torch, I, B, AOS, torch.float32)
    (qdn, _, qdn_guard), (imp, _, imp_guard), (res, _, res_guard) = three_outputs(torch, B, desc.nv, K, AOS, torch.float32)
    with pytest.raises(_lib.MecanoHipError):
        call(hm, D, I, mu, 30, AOS, (qdn, imp, res))
    torch.cuda.synchronize()
    assert b"beyond the range" in _lib.load().mh_last_error()
    for t in (qdn, qdn_guard, imp, imp_guard, res, res_guard):
        assert torch.isnan(t).all()
    call(hm, D, I, [0.5, 3.0e38, 0.5, 0.5], 30, AOS, (qdn, imp, res))  # the largest decade a float holds
    torch.cuda.synchronize()
    assert not torch.isnan(qdn).any() and not torch.isnan(imp).any()
    R = solve(name, I, mu, 30, active=I["active"], v_normal=I["v_normal"])
    label = f"{name} f64 mu={mu}"
    D = device_inputs(torch, I, B, AOS, torch.float64)
    v, p, r = run_poisoned(torch, hm, D, I, mu, 30, AOS, torch.float64, B, desc.nv, label)
    hold_all(v, p, r, I, R, B, desc.n_joints, U64, label)


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("active,v_normal", [(False, True), (True, False)])
def test_active_and_v_normal_are_optional_one_at_a_time(torch_cuda, active, v_normal, layout, dtype_name):
    """The two share their strides: each alone, against the checker, at K = 3."""
    torch = torch_cuda
    dtype, np_dtype, u = precision(torch, dtype_name)
    name = "humanoid30_k3"
    I, _, R = reference(name, dtype_name, mixed_mu(3), 50, active=active, v_normal=v_normal)
    _, desc, om = model_of(name)
    hm = hip_model(desc)
    for B in (65, B_MAX):
        label = f"{name} B={B} layout={layout} {dtype_name} active={active} v_normal={v_normal}"
        D = device_inputs(torch, I, B, layout, dtype)
        v, p, r = run_poisoned(torch, hm, D, I, mixed_mu(3), 50, layout, dtype, B, desc.nv, label, active=active, v_normal=v_normal)
        hold_all(v, p, r, I, R, B, desc.n_joints, u, label, active=active)
        assert np.abs(p).max() > 0.1


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("name", ["arm7", "humanoid30"])
def test_a_contact_that_separates_faster_than_v_normal_gets_exactly_zero_on_the_device(torch_cuda, name, dtype_name):
    """The construction of the CPU test of that name: one contact leaving along its normal at 2 m/s, v_normal = 0.5.  -rho b lies in the
    polar cone from the first sweep on: impulse_out and residual_out are exactly 0; qd_out is qd to the parity bound (the second launch
    adds the forward dynamics of zero wrenches)."""
    torch = torch_cuda
    dtype, np_dtype, u = precision(torch, dtype_name)
    _, desc, om = model_of(name)
    hm, B = hip_model(desc), 65
    I = make_inputs(name, B, dtype=np_dtype)
    tgt, pose, nh = I["targets"][:1], I["poses"][:1], I["normals"][:, :1]
    T = cd.terms(om, desc, I["q"], I["qd"], tgt, pose, nh)
    qd = I["qd"].copy()
    for row in range(B):
        qd[row] += np.linalg.pinv(T["Jl"][row]) @ (2.0 * T["n"][row, 0] - T["Jl"][row] @ qd[row])
    qd = qd.astype(np_dtype).astype(np.float64)
    one = dict(q=I["q"], qd=qd, targets=tgt, poses=pose, normals=nh, active=np.ones((B, 1), dtype=np.int32), v_normal=np.full((B, 1), 0.5), compliance=0.0)
    for mu in (0.0, 0.5):
        R = cd.contact_impulse(om, desc, one["q"], qd, tgt, [mu], pose, nh, None, one["v_normal"], 0.0, 50)
        assert not R["impulse"].any() and not R["residual"].any()
        for layout in (AOS, SOA):
            label = f"{name} layout={layout} {dtype_name} mu={mu} separating"
            D = device_inputs(torch, one, B, layout, dtype)
            v, p, r = run_poisoned(torch, hm, D, one, [mu], 50, layout, dtype, B, desc.nv, label, active=False)
            assert not p.any() and not r.any(), label + ": a separating contact has an impulse or a residual"
            close_aba(v, qd, None, desc.n_joints, u, label=label + " qd+", conds=R["cond_kkt"])


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_a_nan_in_qd_is_nan_in_every_output_of_its_configuration(torch_cuda, layout, dtype_name):
    """One NaN among the velocities of one configuration: its b and with them its impulses are no numbers, and fmax would leave the last
    finite change -- zero -- in residual_out: a configuration that reads as converged.  It is bad like one with a bad trace: NaN in all
    three outputs, every neighbour bit-identical."""
    torch = torch_cuda
    dtype, np_dtype, _ = precision(torch, dtype_name)
    name = "humanoid30"
    _, desc, om = model_of(name)
    hm, B, nan_row = hip_model(desc), 130, 77
    I = wide_inputs(name, B, np_dtype, seed=3)
    I["active"][nan_row] = 1
    D = device_inputs(torch, I, B, layout, dtype)
    good = [t.clone() for t in call(hm, D, I, mixed_mu(4), 10, layout)]
    qd = D["qd"].clone()
    (qd if layout == AOS else qd.t())[nan_row, 2] = float("nan")
    D["qd"] = qd
    got = call(hm, D, I, mixed_mu(4), 10, layout)
    torch.cuda.synchronize()
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[nan_row] = False
    rows = lambda t: t.reshape(B, -1) if layout == AOS or t.dim() == 1 else t.t()
    for g, w in zip(got, good):
        assert not torch.isnan(w).any() and torch.equal(rows(g)[keep], rows(w)[keep]), f"layout={layout} {dtype_name}: a neighbour changed"
    qdn, imp, res = (rows(t)[nan_row] for t in got)
    assert torch.isnan(qdn).all(), "qd_out of the configuration holds numbers"
    finite = bool(torch.isfinite(res).all())  # (torch reads the bits: no compiler flag of the library reaches here)
    assert not (finite and bool(torch.isnan(imp).any())), f"residual_out = {float(res):g} beside NaN impulses: the configuration reads as converged"
    assert torch.isnan(imp).all() and torch.isnan(res).all(), "the header's: NaN in all of its outputs"
