"""mh_rnea_parameters_vjp_* / mh_aba_parameters_vjp_* and the autograd functions on the device against the CPU checker
(tests/parameters_vjp_check.py: the oracle's regressor contracted with the cotangent and chained to (m, c, J), pinned by
tests/test_parameters_vjp_cpu.py) and against the device's own neighbours (regressor, aba_parameters).

Bounds, per configuration.  An entry of the (m, m c, J) gradient is a contraction sum_i u_i Y_ij, so the project's per-entry bound of a
matrix, TOL max(1, |Y|_inf) (helpers.close), sums to |u|_1 TOL max(1, |Y|_inf); the chain rule to (m, c, J) multiplies it by at most
chi = max over the bodies of max(1, m, 1 + |c|_1).  The forward form contracts H^-1 Y with w and takes the per-row bound of
helpers.close_aba in place of TOL: 8 sqrt(8 * 3 n) cond_inf(H(pi_r)) u, cond from the checker's H of the row's own parameters.  fp32:
helpers.f32_forward_tol(3 n) in place of TOL and u = 2^-24, the checker fed the fp32-rounded inputs.  Every check records achieved / bound
(helpers.record_parity)."""
import functools

import numpy as np
import pytest

import inertial_parameters_check as ipc
import parameters_vjp_check as pc
from helpers import close_aba, f32_aba_forward_factor, f32_forward_tol, record_parity
from mecano_amd import random_tools as rt
from test_gravity_gradient_cpu import CASES, GRAVITY, make_case, random_wrenches

pytestmark = pytest.mark.gpu

TOL = 1.0e-10
AOS, SOA = 0, 1
U64, U32 = 2.0 ** -53, 2.0 ** -24
TREE_ROWS = np.array([0, 1, 31, 63, 64, 69])  # (the checker builds three oracle models per body of the 128-body tree)


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def model_of(desc):
    from mecano_amd.engine import HipModel
    return HipModel(desc)


def dev(torch, x, dtype=None):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def soa(x):
    """[B, ...] -> [prod(...), B] contiguous"""
    return None if x is None else x.reshape(x.shape[0], -1).t().contiguous()


def host(t, layout, n=None):
    """The output as an AoS-shaped fp64 array; n: the joints of a parameter-shaped one ([B, n, 10])."""
    if t is None:
        return None
    a = (t.t() if layout == SOA else t).cpu().numpy().astype(np.float64)
    return a if n is None else a.reshape(a.shape[0], n, 10)


def state(sys_, B, seed=5):
    return rt.nextState(np.random.default_rng(seed), sys_, B)


def cotangent(B, nv, seed=8):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, nv))


def parameters(desc, B, seed=4):
    """[B, n, 10]: a different physical parameter set in every row."""
    return ipc.physical_parameter_sets(desc, np.random.default_rng(seed), B)


def inverse(torch, hm, q, qd, qdd, pi, u, layout=AOS, dtype=None, gravity=GRAVITY, **kw):
    """hm.rnea_parameters_vjp on host arrays: gpi [B, n, 10] as an fp64 array."""
    B = q.shape[0]
    args = [dev(torch, None if x is None else np.asarray(x).reshape(B, -1), dtype) for x in (q, qd, qdd, pi, u)]
    if layout == SOA:
        args = [soa(x) for x in args]
    out = hm.rnea_parameters_vjp(*args, gravity, layout, **kw)
    torch.cuda.synchronize()
    return host(out, layout, hm.n_joints)


def forward(torch, hm, q, qd, tau, pi, w, f=None, layout=AOS, dtype=None, gravity=GRAVITY):
    """hm.aba_parameters_vjp on host arrays: (qdd [B, nv], gtau [B, nv], gpi [B, n, 10]) as fp64 arrays."""
    B = q.shape[0]
    args = [dev(torch, None if x is None else np.asarray(x).reshape(B, -1), dtype) for x in (q, qd, tau, pi, w, f)]
    if layout == SOA:
        args = [soa(x) for x in args]
    qdd, gtau, gpi = hm.aba_parameters_vjp(*args[:5], gravity, args[5], layout)
    torch.cuda.synchronize()
    return host(qdd, layout), host(gtau, layout), host(gpi, layout, hm.n_joints)


def held(got, ref, bound, label, rows=None):
    """|got - ref|_inf <= bound per configuration; the worst achieved / bound goes to the parity log."""
    assert got.shape == ref.shape and not np.isnan(got).any(), label
    rows = np.arange(len(ref)) if rows is None else rows
    err = np.abs(got - ref).reshape(len(ref), -1).max(axis=1)
    ratio = float((err[rows] / bound[rows]).max())
    record_parity(ratio, 1.0, label + " achieved / bound")
    print(f"{label}: achieved / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{label}: achieved / bound = {ratio:.3e}"
    return ratio


def inverse_bound(u, scale, chi, tol=TOL):
    return np.abs(u).sum(axis=1) * tol * np.maximum(1.0, scale) * chi


def forward_bound(w, scale, chi, conds, n_joints, unit):
    return np.abs(w).sum(axis=1) * f32_aba_forward_factor(3 * n_joints) * conds * unit * np.maximum(1.0, scale) * chi


# The references of a case are computed once and shared by the layouts (and never written to).  fp32: the checker sees what the device holds.
@functools.lru_cache(maxsize=None)
def case_inputs(case, B=70, single=False):
    sys_, desc = make_case(case)
    q, qd, qdd, tau = state(sys_, B)
    pi, u, w = parameters(desc, B), cotangent(B, desc.nv), cotangent(B, desc.nv, 9)
    f = random_wrenches(np.random.default_rng(21), B, desc.n_joints)
    arrays = (q, qd, qdd, tau, pi, u, w, f)
    if single:
        arrays = tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in arrays)
    return (desc,) + arrays


@functools.lru_cache(maxsize=None)
def inverse_reference(case, single=False):
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case, single=single)
    return pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, GRAVITY)


@functools.lru_cache(maxsize=None)
def forward_reference(case, wrenches, single=False):
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case, single=single)
    return pc.aba_parameters_vjp(desc, q, qd, tau, pi, w, GRAVITY, f if wrenches else None)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", CASES)
def test_fp64_matches_checker(torch_cuda, case, layout):
    """Every model of the gradient tests, both layouts; 70 rows (one full wave and a ragged one), a different parameter set in each."""
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case)
    ref, scale, chi = inverse_reference(case)
    got = inverse(torch_cuda, model_of(desc), q, qd, qdd, pi, u, layout)
    held(got, ref, inverse_bound(u, scale, chi), f"gpi {case} layout {layout}")


@pytest.mark.parametrize("wrenches", [False, True])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", CASES)
def test_forward_fp64_matches_checker(torch_cuda, case, layout, wrenches):
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case)
    qdd_ref, mu_ref, ref, scale, chi, conds = forward_reference(case, wrenches)
    qdd_d, gtau, got = forward(torch_cuda, model_of(desc), q, qd, tau, pi, w, f if wrenches else None, layout)
    close_aba(qdd_d, qdd_ref, None, desc.n_joints, U64, label="qdd", conds=conds)
    close_aba(gtau, mu_ref, None, desc.n_joints, U64, label="gtau", conds=conds)
    held(got, ref, forward_bound(w, scale, chi, conds, desc.n_joints, U64), f"forward gpi {case} layout {layout}")


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_fp32_matches_checker(torch_cuda, case, layout):
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs(case, single=True)
    hm, n = model_of(desc), desc.n_joints
    ref, scale, chi = inverse_reference(case, single=True)
    got = inverse(torch, hm, q, qd, qdd, pi, u, layout, dtype=torch.float32)
    held(got, ref, inverse_bound(u, scale, chi, f32_forward_tol(3 * n)), f"fp32 gpi {case} layout {layout}")
    qdd_ref, mu_ref, ref, scale, chi, conds = forward_reference(case, True, single=True)
    qdd_d, gtau, got = forward(torch, hm, q, qd, tau, pi, w, f, layout, dtype=torch.float32)
    close_aba(qdd_d, qdd_ref, None, n, U32, label=f"fp32 qdd layout {layout}", conds=conds)
    close_aba(gtau, mu_ref, None, n, U32, label=f"fp32 gtau layout {layout}", conds=conds)
    held(got, ref, forward_bound(w, scale, chi, conds, n, U32), f"fp32 forward gpi {case} layout {layout}")


def test_tree128_rows_fp32(torch_cuda):
    """The committed 128-body benchmark tree in fp32 AoS, B = 70: both calls on the rows TREE_ROWS; every row free of NaN."""
    torch = torch_cuda
    sys_ = rt.committedBenchmarkSystems()["tree128"]
    desc = sys_.toModelDesc()
    hm, B, n = model_of(desc), 70, desc.n_joints
    r32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    q, qd, qdd, tau = (r32(x) for x in state(sys_, B))
    pool = r32(parameters(desc, len(TREE_ROWS)))
    pi = pool[np.arange(B) % len(TREE_ROWS)]
    pi[TREE_ROWS] = pool  # a different set in every checked row
    u, w = r32(cotangent(B, desc.nv)), r32(cotangent(B, desc.nv, 9))
    f = r32(random_wrenches(np.random.default_rng(22), B, n))
    got = inverse(torch, hm, q, qd, qdd, pi, u, AOS, dtype=torch.float32)
    ref, scale, chi = pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, GRAVITY, rows=TREE_ROWS)
    held(got, ref, inverse_bound(u, scale, chi, f32_forward_tol(3 * n)), "tree128 gpi", rows=TREE_ROWS)
    qdd_d, gtau, got = forward(torch, hm, q, qd, tau, pi, w, f, AOS, dtype=torch.float32)
    assert np.isfinite(qdd_d).all() and np.isfinite(gtau).all()
    qdd_ref, mu_ref, ref, scale, chi, conds = pc.aba_parameters_vjp(desc, q, qd, tau, pi, w, GRAVITY, f, rows=TREE_ROWS)
    close_aba(qdd_d[TREE_ROWS], qdd_ref[TREE_ROWS], None, n, U32, label="tree128 qdd", conds=conds[TREE_ROWS])
    close_aba(gtau[TREE_ROWS], mu_ref[TREE_ROWS], None, n, U32, label="tree128 gtau", conds=conds[TREE_ROWS])
    held(got, ref, forward_bound(w, scale, chi, conds, n, U32), "tree128 forward gpi", rows=TREE_ROWS)


# ------------------------------------------------------------------------------------------------ ragged and full groups
@functools.lru_cache(maxsize=None)
def arm_pool():
    sys_, desc = make_case("arm7")
    P = 130
    q, qd, qdd, tau = state(sys_, P, seed=15)
    return (desc, q, qd, qdd, tau, parameters(desc, P, 16), cotangent(P, desc.nv, 17))


def padded(torch, shape, pad=96):
    """A NaN-filled buffer with `pad` elements on both sides of a contiguous view of `shape`: (buffer, view)."""
    count = int(np.prod(shape))
    buf = torch.full((count + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda")
    return buf, buf[pad:pad + count].view(*shape)


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_ragged_and_full_groups_write_every_entry_and_nothing_else(torch_cuda, B, layout):
    """The outputs sit in a NaN-poisoned buffer padded on both sides: every entry is written, the padding stays NaN, and every row has
    the bits the same inputs get in a call of 70 rows (the staged AoS store of a ragged group, of a full one, of one row)."""
    torch = torch_cuda
    desc, *pool = arm_pool()
    hm, n, nv, pad = model_of(desc), desc.n_joints, desc.nv, 96
    put = (lambda x: dev(torch, x.reshape(len(x), -1))) if layout == AOS else (lambda x: soa(dev(torch, x.reshape(len(x), -1))))
    back = lambda t: (t if layout == AOS else t.t()).cpu().numpy().reshape(-1, n, 10)

    def run(lo, hi, poisoned):
        q, qd, qdd, tau, pi, u = (put(x[lo:hi]) for x in pool)
        rows = hi - lo
        shape_p, shape_v = ((rows, n * 10), (rows, nv)) if layout == AOS else ((n * 10, rows), (nv, rows))
        bufs = [padded(torch, s, pad) if poisoned else (None, torch.empty(s, dtype=torch.float64, device="cuda")) for s in (shape_p, shape_p, shape_v, shape_v)]
        gi, gf, qdd_o, gtau = (b[1] for b in bufs)
        assert hm.rnea_parameters_vjp(q, qd, qdd, pi, u, GRAVITY, layout, out=gi) is gi
        assert hm.aba_parameters_vjp(q, qd, tau, pi, u, GRAVITY, None, layout, out=(qdd_o, gtau, gf))[2] is gf
        torch.cuda.synchronize()
        for buf, view in bufs:
            assert not torch.isnan(view).any()  # every entry written
            if poisoned:
                assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all()  # nothing outside
        return back(gi), back(gf)

    gi, gf = run(0, B, True)
    lo = max(0, B - 70)
    for first in sorted({0, lo}):
        ref_i, ref_f = run(first, first + 70, False)
        k = min(B - first, 70)
        assert np.array_equal(gi[first:first + k], ref_i[:k]) and np.array_equal(gf[first:first + k], ref_f[:k])


# ------------------------------------------------------------------------------------------------ device against device
@pytest.mark.parametrize("case", ["humanoid30", "planar", "fixed"])
def test_is_the_device_regressor_contracted_and_chained(torch_cuda, case):
    """gpi = chain(u^T regressor(first_moment_columns=True)) with the row's parameters, within the parity bound (the scale from the
    device's own Y)."""
    torch = torch_cuda
    desc, qh, qdh, qddh, tauh, pih, uh, wh, fh = case_inputs(case)
    hm, B, n = model_of(desc), qh.shape[0], desc.n_joints
    q, qd, qdd, u = (dev(torch, x) for x in (qh, qdh, qddh, uh))
    Y = hm.regressor(q, qd, qdd, GRAVITY, first_moment_columns=True)
    ghat = torch.einsum("bi,bij->bj", u, Y).cpu().numpy().reshape(B, n, 10)
    scale = Y.abs().amax(dim=(1, 2)).cpu().numpy()
    got = inverse(torch, hm, qh, qdh, qddh, pih, uh)
    held(got, pc.chain(pih, ghat), inverse_bound(uh, scale, pc.amplification(pih)), f"gpi against the device regressor {case}")


@pytest.mark.parametrize("case", ["arm7", "humanoid30"])
def test_forward_gradient_against_central_differences_of_aba_parameters(torch_cuda, case):
    """For a direction d (a relative change of every number, plus a shift of the centres of mass): <gpi, d> is the central difference of
    w . aba_parameters along d with step 1e-5, to 1e-6 relative; gtau is H(pi_r)^-1 w with the checker's H."""
    torch = torch_cuda
    desc, qh, qdh, qddh, tauh, pih, uh, wh, fh = case_inputs(case)
    hm, B, n = model_of(desc), qh.shape[0], desc.n_joints
    q, qd, tau, w, f = (dev(torch, x) for x in (qh, qdh, tauh, wh, fh))
    rng = np.random.default_rng(41)
    d = pih * rng.uniform(-1.0, 1.0, pih.shape)
    d[..., 1:4] += rng.uniform(-0.01, 0.01, d[..., 1:4].shape)
    h = 1e-5
    up = hm.aba_parameters(q, qd, tau, dev(torch, (pih + h * d).reshape(B, -1)), GRAVITY, f)
    down = hm.aba_parameters(q, qd, tau, dev(torch, (pih - h * d).reshape(B, -1)), GRAVITY, f)
    fd = ((w * (up - down)).sum(1) / (2.0 * h)).cpu().numpy()
    qdd_d, gtau, gpi = forward(torch, hm, qh, qdh, tauh, pih, wh, fh)
    lhs = (gpi * d).reshape(B, -1).sum(1)
    err = np.abs(lhs - fd) / np.maximum(1.0, np.abs(fd))
    record_parity(err.max(), 1e-6, f"<gpi, d> against central differences {case}")
    print(f"{case}: worst relative difference {err.max():.3e}")
    assert err.max() <= 1e-6
    H = ipc.Checker(desc).crba(qh, pih)
    conds = np.array([np.linalg.cond(Hr, np.inf) for Hr in H])
    close_aba(gtau, np.linalg.solve(H, wh[..., None])[..., 0], None, n, U64, label="gtau against the checker's H", conds=conds)
    assert np.array_equal(qdd_d, hm.aba_parameters(q, qd, tau, dev(torch, pih.reshape(B, -1)), GRAVITY, f).cpu().numpy())


# ------------------------------------------------------------------------------------------------ structure
def subtree_of(desc, j):
    inside = np.zeros(desc.n_joints, dtype=bool)
    inside[j] = True
    changed = True
    while changed:  # (no order of the listing is assumed)
        changed = False
        for k in range(desc.n_joints):
            p = int(desc.parent[k])
            if p >= 0 and inside[p] and not inside[k]:
                inside[k] = changed = True
    return inside


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_blocks_outside_the_subtree_of_the_only_loaded_joint_are_zero(torch_cuda, layout):
    """u non-zero at one joint only: nu is zero outside that joint's subtree, and so is -- exactly -- every block there; u = 0 gives
    zeros everywhere, in the forward form (w = 0) too."""
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs("humanoid30")
    hm, n = model_of(desc), desc.n_joints
    kids = np.bincount(np.asarray(desc.parent)[np.asarray(desc.parent) >= 0], minlength=n)
    ofs = np.concatenate([[0], np.cumsum([{0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}[int(t)] for t in desc.joint_type])])
    picked = [j for j in range(n) if desc.parent[j] >= 0 and kids[j] > 0][:3]
    assert picked
    for j in picked:
        one = np.zeros_like(u)
        cols = np.asarray(desc.dof_indices)[ofs[j]:ofs[j + 1]]
        one[:, cols] = u[:, cols]
        got = inverse(torch, hm, q, qd, qdd, pi, one, layout)
        inside = subtree_of(desc, j)
        assert 0 < inside.sum() < n
        assert not got[:, ~inside].any(), j       # exactly 0.0
        assert np.abs(got[:, inside]).reshape(len(got), inside.sum(), 10).max(axis=2).min() > 0.0, j  # and every block inside is not
    assert not inverse(torch, hm, q, qd, qdd, pi, np.zeros_like(u), layout).any()
    assert not forward(torch, hm, q, qd, tau, pi, np.zeros_like(w), f, layout)[2].any()


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_only_the_changed_rows_change_and_bad_rows_stay_alone(torch_cuda, layout):
    """Another parameter set in one row changes that row only (bit for bit elsewhere); a NaN in pi or a massless row is not finite in
    its own row alone, and the call returns MH_OK."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, k = model_of(desc), 130, 64
    q, qd, qdd, tau = state(sys_, B)
    pi, u = parameters(desc, B), cotangent(B, desc.nv)
    keep = np.arange(B) != k
    gi = inverse(torch, hm, q, qd, qdd, pi, u, layout)
    qdd_f, gtau, gf = forward(torch, hm, q, qd, tau, pi, u, None, layout)
    other = pi.copy()
    other[k] = parameters(desc, 1, 99)[0]
    gi2 = inverse(torch, hm, q, qd, qdd, other, u, layout)
    qdd_f2, gtau2, gf2 = forward(torch, hm, q, qd, tau, other, u, None, layout)
    for a, b in ((gi, gi2), (gf, gf2), (qdd_f, qdd_f2), (gtau, gtau2)):
        assert np.array_equal(a[keep], b[keep]) and np.abs(a[k] - b[k]).max() > 1e-6
    nan_row = pi.copy()
    nan_row[k, 3, 0] = np.nan
    gi3 = inverse(torch, hm, q, qd, qdd, nan_row, u, layout)
    assert not np.isfinite(gi3[k]).all() and np.array_equal(gi3[keep], gi[keep])
    massless = pi.copy()
    massless[k] = 0.0
    qdd_f3, gtau3, gf3 = forward(torch, hm, q, qd, tau, massless, u, None, layout)
    assert not np.isfinite(gf3[k]).all() and not np.isfinite(qdd_f3[k]).all()
    for a, b in ((gf, gf3), (qdd_f, qdd_f3), (gtau, gtau3)):
        assert np.isfinite(b[keep]).all() and np.array_equal(a[keep], b[keep])


def test_fixed_joints_bodies_get_a_block(torch_cuda):
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs("fixed")
    fixed = [j for j in range(desc.n_joints) if int(desc.joint_type[j]) == 3 and desc.parent[j] >= 0]
    assert fixed, "the model has fixed joints below a moving one"
    got = inverse(torch_cuda, model_of(desc), q, qd, qdd, pi, u)
    ref = inverse_reference("fixed")[0]
    assert np.abs(ref[:, fixed]).max() > 1e-3 and np.abs(got[:, fixed]).max() > 1e-3


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
def test_a_model_without_dofs_gets_exact_zero_blocks(torch_cuda, layout, dtype_name):
    """Fixed joints only, nv = 0, through the C ABI (the state matrices are empty; the call wants pointers all the same): the forward
    form has no forward dynamics to run and does not return early -- it writes gpi, a zero block for every body (qdd does not depend
    on pi), over what the output held, with qdd_out and gtau_out NULL."""
    import ctypes

    from mecano_amd import _lib
    from mecano_amd.multibody import MultiBodySystem
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    joints = rt.nextJointTree(np.random.default_rng(3), 3, ("fixed",))
    desc = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor()).toModelDesc()
    assert desc.nv == 0 and desc.nq == 0
    hm, B, n = model_of(desc), 65, desc.n_joints
    pi = dev(torch, parameters(desc, B).reshape(B, -1), dtype)
    gpi = torch.full((B, 10 * n), float("nan"), dtype=dtype, device="cuda")
    if layout == SOA:
        pi, gpi = soa(pi), soa(gpi)
    q, qd, tau, w = (torch.zeros(8, dtype=dtype, device="cuda") for _ in range(4))  # somewhere to point: nothing of them is read
    g, ra = hm._root(GRAVITY)
    opts = hm._options(layout, True, True, torch.cuda.current_stream().cuda_stream, root_acceleration=ra)
    _lib.check(getattr(_lib.load(), "mh_aba_parameters_vjp_" + ("f64" if dtype_name == "float64" else "f32"))(
        hm._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), pi.data_ptr(), g, None, w.data_ptr(), ctypes.byref(opts), None, None, gpi.data_ptr()))
    torch.cuda.synchronize()
    assert not torch.isnan(gpi).any() and not gpi.any()


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case,B", [("arm7", 1), ("arm7", 65), ("humanoid30", 197)])
def test_forward_form_outputs_in_scratch_and_both_switches_on(torch_cuda, case, B, layout, dtype_name):
    """qdd and gtau None (both in the context's scratch), each alone, and the call through the C ABI with consider_coriolis = 0 and
    consider_accelerations = 0 (the per-row form runs everything with both switches on): gpi has the bits of the full call."""
    import ctypes

    from mecano_amd import _lib
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    sys_, desc = make_case(case)
    hm, n, nv = model_of(desc), desc.n_joints, desc.nv
    q, qd, _, tau = state(sys_, B)
    pi, w = parameters(desc, B), cotangent(B, nv, 9)
    f = random_wrenches(np.random.default_rng(21), B, n)
    put = lambda x: dev(torch, x.reshape(B, -1), dtype) if layout == AOS else soa(dev(torch, x.reshape(B, -1), dtype))
    Q, QD, TAU, PI, W, F = (put(x) for x in (q, qd, tau, pi, w, f))
    full = hm.aba_parameters_vjp(Q, QD, TAU, PI, W, GRAVITY, F, layout)
    assert all(torch.isfinite(t).all() for t in full) and full[2].any()
    for keep in ((2,), (0, 2), (1, 2)):  # of (qdd, gtau, gpi)
        outs = tuple(torch.full_like(t, float("nan")) if k in keep else None for k, t in enumerate(full))
        res = hm.aba_parameters_vjp(Q, QD, TAU, PI, W, GRAVITY, F, layout, out=outs)
        torch.cuda.synchronize()
        assert all((r is None) if k not in keep else torch.equal(r, full[k]) for k, r in enumerate(res)), keep
    outs = [torch.full_like(t, float("nan")) for t in full]
    g, ra = hm._root(GRAVITY)
    opts = hm._options(layout, False, False, torch.cuda.current_stream().cuda_stream, root_acceleration=ra)
    _lib.check(getattr(_lib.load(), "mh_aba_parameters_vjp_" + ("f64" if dtype_name == "float64" else "f32"))(
        hm._h, B, Q.data_ptr(), QD.data_ptr(), TAU.data_ptr(), PI.data_ptr(), g, F.data_ptr(), W.data_ptr(), ctypes.byref(opts),
        *(o.data_ptr() for o in outs)))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, full))


def test_switches_and_root_acceleration(torch_cuda):
    """consider_coriolis = False gives the bits of qd = 0 and needs no qd; consider_accelerations = False those of qdd = 0; a root
    acceleration (0, -g) gives the bits of the gravity vector g.  The checker agrees with each."""
    torch = torch_cuda
    desc, q, qd, qdd, tau, pi, u, w, f = case_inputs("humanoid30")
    hm = model_of(desc)
    z = np.zeros_like(qd)
    for layout in (AOS, SOA):
        no_c = inverse(torch, hm, q, None, qdd, pi, u, layout, consider_coriolis=False)
        assert np.array_equal(no_c, inverse(torch, hm, q, z, qdd, pi, u, layout))
        assert np.array_equal(no_c, inverse(torch, hm, q, qd, qdd, pi, u, layout, consider_coriolis=False))
        no_a = inverse(torch, hm, q, qd, None, pi, u, layout, consider_accelerations=False)
        assert np.array_equal(no_a, inverse(torch, hm, q, qd, z, pi, u, layout))
        none = inverse(torch, hm, q, None, None, pi, u, layout, consider_coriolis=False, consider_accelerations=False)
        assert np.array_equal(none, inverse(torch, hm, q, z, z, pi, u, layout))
        root = np.concatenate([np.zeros(3), -np.asarray(GRAVITY)])
        assert np.array_equal(inverse(torch, hm, q, qd, qdd, pi, u, layout, gravity=root), inverse(torch, hm, q, qd, qdd, pi, u, layout))
        assert np.array_equal(forward(torch, hm, q, qd, tau, pi, w, f, layout, gravity=root)[2], forward(torch, hm, q, qd, tau, pi, w, f, layout)[2])
    ref, scale, chi = pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, GRAVITY, False, True)
    held(no_c, ref, inverse_bound(u, scale, chi), "gpi without Coriolis terms")
    ref, scale, chi = pc.rnea_parameters_vjp(desc, q, qd, qdd, pi, u, GRAVITY, True, False)
    held(no_a, ref, inverse_bound(u, scale, chi), "gpi without accelerations")
    assert np.abs(no_c - no_a).max() > 1e-3


def test_custom_index_provider_and_listing_order(torch_cuda):
    """State rows and cotangents follow the model's index maps; pi and gpi follow the LISTING order of the joints."""
    torch = torch_cuda
    from mecano_amd.multibody import ModelDesc, MultiBodySystem
    rng = np.random.default_rng(31)
    sys_ = MultiBodySystem.toMultiBodySystemInput(rt.nextJointTree(rng, 12, ("revolute", "prismatic"))[0].getPredecessor())
    d = sys_.toModelDesc()
    n, B = d.n_joints, 70
    q, qd, qdd, tau = state(sys_, B)
    pi, u = parameters(d, B), cotangent(B, d.nv)
    ref_i, scale, chi = pc.rnea_parameters_vjp(d, q, qd, qdd, pi, u, GRAVITY)
    qdd_ref, mu_ref, ref_f, scale_f, chi_f, conds = pc.aba_parameters_vjp(d, q, qd, tau, pi, u, GRAVITY)
    bi, bf = inverse_bound(u, scale, chi), forward_bound(u, scale_f, chi_f, conds, n, U64)
    perm = rng.permutation(d.nv).astype(np.int32)  # joint k now owns matrix row perm[k] (and configuration entry perm[k])
    d1 = sys_.toModelDesc()
    d1.dof_indices, d1.cfg_indices = perm.copy(), perm.copy()

    def moved(x):
        y = np.zeros_like(x)
        y[:, perm] = x
        return y

    hm1 = model_of(d1)
    held(inverse(torch, hm1, moved(q), moved(qd), moved(qdd), pi, moved(u), AOS), ref_i, bi, "permuted map: gpi")
    qdd_d, gtau, got = forward(torch, hm1, moved(q), moved(qd), moved(tau), pi, moved(u), None, SOA)
    close_aba(qdd_d[:, perm], qdd_ref, None, n, U64, label="permuted map: qdd", conds=conds)
    close_aba(gtau[:, perm], mu_ref, None, n, U64, label="permuted map: gtau", conds=conds)
    held(got, ref_f, bf, "permuted map: forward gpi")
    order = rng.permutation(n)  # another listing order of the joints, same rows: the blocks move with the joints
    inv = np.argsort(order)
    r = lambda a, w: np.asarray(a).reshape(n, w)[order].reshape(-1)
    parent = np.array([(-1 if d.parent[o] < 0 else inv[d.parent[o]]) for o in order], dtype=np.int32)
    d2 = ModelDesc(n, d.nq, d.nv, parent, np.asarray(d.joint_type)[order], r(d.axis, 3), r(d.X_before, 12), r(d.X_com, 12), r(d.inertia_J, 9),
                   np.asarray(d.inertia_mass)[order], r(d.inertia_com, 3), np.asarray(d.dof_indices)[order], np.asarray(d.cfg_indices)[order])
    hm2 = model_of(d2)
    held(inverse(torch, hm2, q, qd, qdd, pi[:, order], u, SOA), ref_i[:, order], bi, "another listing order: gpi")
    held(forward(torch, hm2, q, qd, tau, pi[:, order], u, None, AOS)[2], ref_f[:, order], bf, "another listing order: forward gpi")


# ------------------------------------------------------------------------------------------------ plumbing
def test_two_contexts_on_two_streams_and_out_reuse(torch_cuda):
    """Two context views, each on a stream of its own, give the default context's bits; `out=` is written in place and reused."""
    torch = torch_cuda
    desc, qh, qdh, qddh, tauh, pih, uh, wh, fh = case_inputs("humanoid30")
    hm, B = model_of(desc), qh.shape[0]
    q, qd, qdd, tau, u, f = (dev(torch, x) for x in (qh, qdh, qddh, tauh, uh, fh))
    pi = dev(torch, pih)
    ref_i = hm.rnea_parameters_vjp(q, qd, qdd, pi, u, GRAVITY)
    ref_f = hm.aba_parameters_vjp(q, qd, tau, pi, u, GRAVITY, f)
    torch.cuda.synchronize()
    views, streams = [hm.context(), hm.context()], [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for view, s in zip(views, streams):
        view.reserve(B)
        gi, gf = torch.empty_like(ref_i), torch.empty_like(ref_f[2])
        with torch.cuda.stream(s):
            for _ in range(2):  # the second call reuses the outputs
                assert view.rnea_parameters_vjp(q, qd, qdd, pi, u, GRAVITY, out=gi) is gi
                res = view.aba_parameters_vjp(q, qd, tau, pi, u, GRAVITY, f, out=(None, None, gf))  # qdd, mu: the context's scratch
                assert res[0] is None and res[1] is None and res[2] is gf
        outs.append((gi, gf))
    for view, s, (gi, gf) in zip(views, streams, outs):
        view.check(s.cuda_stream)
        assert torch.equal(gi, ref_i) and torch.equal(gf, ref_f[2])
        view.close()


def test_forward_form_replays_from_a_graph(torch_cuda):
    """After reserve() and a first call the forward form is captured into one graph on one stream (it only enqueues work) and the replay
    gives the bits of the direct call, also on changed inputs."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = model_of(desc), 1000
    q, qd, _, tau = (dev(torch, x) for x in state(sys_, B))
    w = dev(torch, cotangent(B, desc.nv, 9))
    pool = parameters(desc, 50)
    pi = dev(torch, pool[np.arange(B) % 50])
    f = dev(torch, random_wrenches(np.random.default_rng(26), B, desc.n_joints))
    ref = hm.aba_parameters_vjp(q, qd, tau, pi, w, GRAVITY, f)
    torch.cuda.synchronize()
    view = hm.context()
    view.reserve(B)
    gpi = torch.empty_like(ref[2])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        view.aba_parameters_vjp(q, qd, tau, pi, w, GRAVITY, f, out=(None, None, gpi))
        view.check(s.cuda_stream)
        assert torch.equal(gpi, ref[2])
        gpi.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            view.aba_parameters_vjp(q, qd, tau, pi, w, GRAVITY, f, out=(None, None, gpi))
    torch.cuda.synchronize()
    assert not gpi.any()  # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gpi, ref[2])
    pi2, w2 = dev(torch, pool[(np.arange(B) + 7) % 50]), dev(torch, cotangent(B, desc.nv, 14))
    ref2 = hm.aba_parameters_vjp(q, qd, tau, pi2, w2, GRAVITY, f)
    pi.copy_(pi2), w.copy_(w2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gpi, ref2[2]) and not torch.equal(ref2[2], ref[2])
    view.close()


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_is_the_method_and_a_shared_pi_gets_the_row_sum(torch_cuda):
    """torch.autograd.grad of sum(w * f(pi)) is the method's gpi bit for bit, in either shape of pi; a pi made by
    shared.expand(B, n, 10).contiguous() hands the sum over the rows to `shared`; a state that requires grad raises
    NotImplementedError in the forward; a second backward raises."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    desc, qh, qdh, qddh, tauh, pih, uh, wh, fh = case_inputs("humanoid30")
    hm, B, n = model_of(desc), qh.shape[0], desc.n_joints
    q, qd, qdd, tau, w, f = (dev(torch, x) for x in (qh, qdh, qddh, tauh, wh, fh))
    for fn, x3, direct in ((mha.rnea_parameters, qdd, lambda p: hm.rnea_parameters_vjp(q, qd, qdd, p, w, GRAVITY)),
                           (mha.aba_parameters, tau, lambda p: hm.aba_parameters_vjp(q, qd, tau, p, w, GRAVITY, f)[2])):
        for shape in ((B, n, 10), (B, n * 10)):
            pi = dev(torch, pih.reshape(shape)).requires_grad_()
            out = fn(hm, q, qd, x3, pi, GRAVITY, f)
            assert out.shape == (B, desc.nv)
            (got,) = torch.autograd.grad((w * out).sum(), (pi,))
            assert got.shape == shape and torch.equal(got, direct(pi.detach()))
        shared = dev(torch, pih[0]).requires_grad_()
        pi = shared.expand(B, n, 10).contiguous()
        (got,) = torch.autograd.grad((w * fn(hm, q, qd, x3, pi, GRAVITY, f)).sum(), (shared,))
        rows = direct(pi.detach())
        assert got.shape == (n, 10) and torch.allclose(got, rows.sum(0), rtol=1e-12, atol=1e-12 * float(rows.abs().max()) * B)
        for k in range(3):  # a state that requires grad
            args = [q, qd, x3]
            args[k] = args[k].clone().requires_grad_()
            with pytest.raises(NotImplementedError):
                fn(hm, *args, dev(torch, pih), GRAVITY, f)
        pi = dev(torch, pih).requires_grad_()
        (g1,) = torch.autograd.grad((w * fn(hm, q, qd, x3, pi, GRAVITY, f)).sum(), (pi,), create_graph=True)
        with pytest.raises(RuntimeError):
            g1.sum().backward()


def test_gradcheck_on_the_arm(torch_cuda):
    """torch.autograd.gradcheck of both functions with respect to pi: arm7, fp64, B = 3.  Its central difference with eps = 1e-6: the
    efforts are linear in every single number (no truncation) and round to |tau| 2^-53 / eps, about 1e-8; the accelerations round to
    cond(H) 2^-53 |qdd| / eps, about 1e-6 at cond 1e2 and |qdd| 1e2, beside a truncation of eps^2 times the third derivative -- hence
    1e-6 absolute + 1e-5 relative for the inverse dynamics and ten times that for the forward dynamics."""
    from mecano_amd import autograd as mha
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B = model_of(desc), 3
    q, qd, qdd, tau = (dev(torch, x) for x in state(sys_, B))
    pi = dev(torch, parameters(desc, B)).requires_grad_()
    assert torch.autograd.gradcheck(lambda p: mha.rnea_parameters(hm, q, qd, qdd, p, GRAVITY), (pi,), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda p: mha.aba_parameters(hm, q, qd, tau, p, GRAVITY), (pi,), eps=1e-6, atol=1e-5, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ example
def test_the_identification_example_lowers_its_loss(torch_cuda):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "identify_by_simulation_error.py")
    spec = importlib.util.spec_from_file_location("identify_by_simulation_error", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after, unseen = mod.main(samples=256, iterations=5)
    assert np.isfinite([before, after, unseen]).all() and after < before
