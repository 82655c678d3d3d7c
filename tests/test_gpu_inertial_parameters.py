"""mh_rnea_parameters_* / mh_aba_parameters_* on the device against the CPU checker (tests/inertial_parameters_check.py: one C-oracle
model per distinct parameter set), with the project's own tolerances (tests/helpers.py)."""
import ctypes

import numpy as np
import pytest

import inertial_parameters_check as ipc
from helpers import (DistinctRows, check_bad_outputs, check_cover, close, close_aba, f32_aba_backward_tol, f32_forward_tol, group_cover,
                     poisoned, record_parity)
from test_inertial_parameters_cpu import CASES, GRAVITY, batch, make_case

pytestmark = pytest.mark.gpu
AOS, SOA = 0, 1
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, x, dtype=None):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype or torch.float64)


def model_of(desc):
    from mecano_amd.engine import HipModel
    return HipModel(desc)


def run(torch, hm, kind, q, qd, x3, pi, layout, f=None, dtype=None, **kw):
    """rnea_parameters / aba_parameters of host arrays in `layout`; returns [B, nv] on the host (fp64)."""
    B = q.shape[0]
    put = (lambda x: dev(torch, x, dtype)) if layout == AOS else (lambda x: dev(torch, np.asarray(x).reshape(B, -1).T, dtype))
    fn = hm.rnea_parameters if kind == "rnea" else hm.aba_parameters
    out = fn(put(q), put(qd), put(x3), put(np.asarray(pi).reshape(B, -1)), GRAVITY, None if f is None else put(f), layout, **kw)
    torch.cuda.synchronize()
    out = out if layout == AOS else out.t()
    return out.cpu().numpy().astype(np.float64)


def wrenches(B, n, seed=9):
    return np.random.default_rng(seed).uniform(-5.0, 5.0, (B, n, 6))


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", CASES)
def test_fp64_parity_with_the_checker(torch_cuda, case, layout):
    """tau within close(1e-10); qdd within close_aba's per-row bound with cond_inf of each row's OWN H.  With and without wrenches."""
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, ck, B = model_of(desc), ipc.Checker(desc), 70
    q, qd, qdd, tau, pi = batch(sys_, desc, B)
    H = ck.crba(q, pi)
    for f in (None, wrenches(B, desc.n_joints)):
        tag = f"{case} {'soa' if layout else 'aos'} {'f_ext' if f is not None else 'free'}"
        got = run(torch, hm, "rnea", q, qd, qdd, pi, layout, f)
        err = close(got, ck.rnea(q, qd, qdd, pi, GRAVITY, f), 1e-10, label="rnea_parameters " + tag)
        got_a = run(torch, hm, "aba", q, qd, tau, pi, layout, f)
        ratio = close_aba(got_a, ck.aba(q, qd, tau, pi, GRAVITY, f), H, desc.n_joints, label="aba_parameters " + tag)
        print(f"{tag}: rnea err {err:.3e}, aba err / (cond u) {ratio:.3e}")
    for cc, ca in ((False, True), (True, False), (False, False)):  # the two switches of the inverse dynamics (Checker.rnea: Coriolis off = qd = 0)
        got = run(torch, hm, "rnea", q, qd, qdd, pi, layout, consider_coriolis=cc, consider_accelerations=ca)
        close(got, ck.rnea(q, qd, qdd, pi, GRAVITY, None, cc, ca), 1e-10, label=f"rnea_parameters {case} switches {cc} {ca}")


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("case", CASES)
def test_fp32_against_the_fp64_checker(torch_cuda, case, layout):
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, ck, B, n = model_of(desc), ipc.Checker(desc), 70, desc.n_joints
    q, qd, qdd, tau, pi = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in batch(sys_, desc, B))  # what the device holds
    t32 = run(torch, hm, "rnea", q, qd, qdd, pi, layout, dtype=torch.float32)
    close(t32, ck.rnea(q, qd, qdd, pi, GRAVITY), f32_forward_tol(n), label=f"rnea_parameters_f32 {case}")
    a32 = run(torch, hm, "aba", q, qd, tau, pi, layout, dtype=torch.float32)
    assert np.isfinite(a32).all()
    a_ref = ck.aba(q, qd, tau, pi, GRAVITY)
    bias = ck.rnea(q, qd, np.zeros_like(qdd), pi, GRAVITY)
    back = ck.rnea(q, qd, a32, pi, GRAVITY)  # exact (fp64) inverse dynamics of the fp32 answer, row by row with the row's parameters
    scale = np.abs(tau).max() + np.abs(bias).max()
    berr = np.abs(back - tau).max()
    record_parity(berr, f32_aba_backward_tol(n) * scale, f"aba_parameters_f32 backward error {case}")
    print(f"{case}: fp32 backward error {berr:.3e} (bound {f32_aba_backward_tol(n) * scale:.3e})")
    assert berr <= f32_aba_backward_tol(n) * scale, (berr, scale)
    close_aba(a32, a_ref, ck.crba(q, pi), n, u=U32, label=f"aba_parameters_f32 {case}")


@pytest.mark.parametrize("case", CASES)
def test_own_parameters_reproduce_the_fixed_parameter_calls(torch_cuda, case):
    """mh_model_inertial_parameters in every row: mh_rnea_* / mh_aba_* within the same tolerances (the device maps the ten numbers to its
    inertia record in the precision of the call, the host did it once in fp64: not the same bits)."""
    torch = torch_cuda
    from oracle.cpu_oracle import OracleModel
    sys_, desc = make_case(case)
    hm, B = model_of(desc), 200
    q, qd, qdd, tau, _ = batch(sys_, desc, B)
    own = np.broadcast_to(hm.inertial_parameters(), (B, desc.n_joints, 10))
    f = wrenches(B, desc.n_joints)
    tq, tqd, tqdd, ttau, tf = (dev(torch, x) for x in (q, qd, qdd, tau, f))
    close(run(torch, hm, "rnea", q, qd, qdd, own, AOS, f), hm.rnea(tq, tqd, tqdd, GRAVITY, tf).cpu().numpy(), 1e-10, label=f"own rnea {case}")
    close_aba(run(torch, hm, "aba", q, qd, tau, own, SOA, f), hm.aba(tq, tqd, ttau, GRAVITY, tf).cpu().numpy(), OracleModel(desc).crba(q),
              desc.n_joints, label=f"own aba {case}")
    for cc, ca in ((False, True), (True, False)):  # the switches behave as in mh_rnea_*
        close(run(torch, hm, "rnea", q, qd, qdd, own, AOS, consider_coriolis=cc, consider_accelerations=ca),
              hm.rnea(tq, tqd, tqdd, GRAVITY, consider_coriolis=cc, consider_accelerations=ca).cpu().numpy(), 1e-10, label=f"own rnea {case} switches {cc} {ca}")


@pytest.mark.parametrize("case", ["humanoid30", "mixed"])
def test_inverse_dynamics_is_the_regressor_times_the_parameters(torch_cuda, case):
    """On the device: rnea_parameters = regressor(first_moment_columns=True) @ (m, m c, J), row by row."""
    torch = torch_cuda
    sys_, desc = make_case(case)
    hm, B = model_of(desc), 300
    q, qd, qdd, _, pi = batch(sys_, desc, B)
    Y = hm.regressor(dev(torch, q), dev(torch, qd), dev(torch, qdd), GRAVITY, first_moment_columns=True)
    ref = torch.einsum("bij,bj->bi", Y, dev(torch, ipc.first_moment_form(pi).reshape(B, -1))).cpu().numpy()
    close(run(torch, hm, "rnea", q, qd, qdd, pi, AOS), ref, 1e-10, label=f"Y pi {case}")


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_only_the_changed_rows_outputs_change(torch_cuda, layout):
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, k = model_of(desc), 130, 77
    q, qd, qdd, tau, pool = batch(sys_, desc, B)
    other = ipc.physical_parameter_sets(desc, np.random.default_rng(99), 1)[0]
    for kind, x3 in (("rnea", qdd), ("aba", tau)):
        first = run(torch, hm, kind, q, qd, x3, pool, layout)
        changed = pool.copy()
        changed[k] = other
        second = run(torch, hm, kind, q, qd, x3, changed, layout)
        keep = np.arange(B) != k
        assert np.array_equal(first[keep], second[keep]), kind  # bit for bit elsewhere
        assert np.abs(first[k] - second[k]).max() > 1e-6, kind


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("B", [262144, 2 * 8 * 256 * 64 + 64 + 37])
def test_device_filling_batch_covers_every_row_group(torch_cuda, layout, B):
    """Every lane loops over several groups of 64 rows; the ragged size ends in a partly filled group (the lanes still in the loop share
    the staged read of pi).  DistinctRows states, parameter sets from a pool of 61 -- a prime: the pool's period divides no
    group stride --, outputs poisoned with a guard row, rows sampled with group_cover, none of them left out of the comparison."""
    torch = torch_cuda
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    sys_, desc = make_case("humanoid30")
    hm, ck, nv, n = model_of(desc), ipc.Checker(desc), desc.nv, desc.n_joints
    rows = DistinctRows(sys_, 256, seed=31)
    tq, tqd, tqdd, ttau = rows.device(torch, B)
    pool = ipc.physical_parameter_sets(desc, np.random.default_rng(61), 61).reshape(61, -1)
    tpi = dev(torch, pool)[torch.arange(B, device="cuda") % 61].contiguous()
    idx = group_cover(B, 8 * cus)
    q, qd, qdd, tau = rows.rows(idx)
    pi = pool[idx % 61]
    put = (lambda x: x) if layout == AOS else (lambda x: x.t().contiguous())
    for kind, x3 in (("rnea", tqdd), ("aba", ttau)):
        if layout == AOS:
            out, guard = poisoned(torch, B, (nv,), torch.float64)
            view = out
        else:
            out, guard = poisoned(torch, nv, (B,), torch.float64)
            view = out.t()
        fn = hm.rnea_parameters if kind == "rnea" else hm.aba_parameters
        assert fn(put(tq), put(tqd), put(x3), put(tpi), GRAVITY, None, layout, out=out) is out
        torch.cuda.synchronize()
        if kind == "rnea":
            check_cover(view, guard, idx, ck.rnea(q, qd, qdd, pi, GRAVITY), 1e-10, label=f"rnea_parameters B={B}")
        else:
            assert torch.isnan(guard).all() and not torch.isnan(view).any()  # nothing past the last row, no row left unwritten
            got = view[torch.as_tensor(idx, device="cuda")].cpu().numpy()
            assert got.shape[0] == len(idx)  # no sampled row is left out
            close_aba(got, ck.aba(q, qd, tau, pi, GRAVITY), ck.crba(q, pi), n, label=f"aba_parameters B={B}")


def test_custom_index_provider_and_listing_order(torch_cuda):
    """State rows follow the model's index maps; pi follows the LISTING order of the joints, whatever order the kernels walk in."""
    torch = torch_cuda
    from mecano_amd import random_tools as rt
    from mecano_amd.multibody import ModelDesc, MultiBodySystem
    rng = np.random.default_rng(31)
    sys_ = MultiBodySystem.toMultiBodySystemInput(rt.nextJointTree(rng, 12, ("revolute", "prismatic"))[0].getPredecessor())
    d = sys_.toModelDesc()
    n, B = d.n_joints, 70
    q, qd, qdd, tau, pi = batch(sys_, d, B)
    ck = ipc.Checker(d)
    ref_t, ref_a, H = ck.rnea(q, qd, qdd, pi, GRAVITY), ck.aba(q, qd, tau, pi, GRAVITY), ck.crba(q, pi)
    # joint k now owns matrix row perm[k] (and configuration entry perm[k])
    perm = rng.permutation(d.nv).astype(np.int32)
    d1 = sys_.toModelDesc()
    d1.dof_indices, d1.cfg_indices = perm.copy(), perm.copy()

    def moved(x):
        y = np.zeros_like(x)
        y[:, perm] = x
        return y

    hm1 = model_of(d1)
    close(run(torch, hm1, "rnea", moved(q), moved(qd), moved(qdd), pi, AOS)[:, perm], ref_t, 1e-10, label="permuted map: rnea")
    close_aba(run(torch, hm1, "aba", moved(q), moved(qd), moved(tau), pi, SOA)[:, perm], ref_a, H, n, label="permuted map: aba")
    # another listing order of the joints, same rows: the blocks of pi move with the joints
    order = rng.permutation(n)
    inv = np.argsort(order)
    r = lambda a, w: np.asarray(a).reshape(n, w)[order].reshape(-1)
    parent = np.array([(-1 if d.parent[o] < 0 else inv[d.parent[o]]) for o in order], dtype=np.int32)
    d2 = ModelDesc(n, d.nq, d.nv, parent, np.asarray(d.joint_type)[order], r(d.axis, 3), r(d.X_before, 12), r(d.X_com, 12), r(d.inertia_J, 9),
                   np.asarray(d.inertia_mass)[order], r(d.inertia_com, 3), np.asarray(d.dof_indices)[order], np.asarray(d.cfg_indices)[order])
    hm2 = model_of(d2)
    assert np.array_equal(hm2.inertial_parameters(), ipc.parameters_of(d)[order])
    pi2 = pi.reshape(B, n, 10)[:, order]
    close(run(torch, hm2, "rnea", q, qd, qdd, pi2, SOA), ref_t, 1e-10, label="another listing order: rnea")
    close_aba(run(torch, hm2, "aba", q, qd, tau, pi2, AOS), ref_a, H, n, label="another listing order: aba")


def test_fixed_joints_carry_inertia(torch_cuda):
    """Changing only the block of a FIXED joint's successor changes the efforts of its ancestors (and matches the checker)."""
    torch = torch_cuda
    sys_, desc = make_case("mixed")
    fixed = [j for j in range(desc.n_joints) if int(desc.joint_type[j]) == 3]
    assert fixed, "the mixed tree has fixed joints"
    hm, ck, B = model_of(desc), ipc.Checker(desc), 66
    q, qd, qdd, tau, pi = batch(sys_, desc, B)
    base = run(torch, hm, "rnea", q, qd, qdd, pi, AOS)
    heavy = pi.copy()
    heavy[:, fixed, 0] *= 3.0
    heavy[:, fixed, 4:] *= 3.0
    got = run(torch, hm, "rnea", q, qd, qdd, heavy, AOS)
    close(got, ck.rnea(q, qd, qdd, heavy, GRAVITY), 1e-10, label="fixed joints' blocks")
    assert np.abs(got - base).max() > 1e-3


def test_contexts_two_streams_out_reuse_and_graph(torch_cuda):
    """A context on a stream of its own gives the default context's bits; `out=` is written in place and reused; after reserve() and one
    first call the call is captured into a graph (it only enqueues work) and the replay equals the eager call."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B = model_of(desc), 1000
    q, qd, qdd, tau, pool = batch(sys_, desc, 50)
    tile = lambda x: dev(torch, np.tile(x.reshape(50, -1), (B // 50, 1)))
    tq, tqd, tqdd, ttau, tpi = tile(q), tile(qd), tile(qdd), tile(tau), tile(pool)
    for layout in (AOS, SOA):
        put = (lambda x: x) if layout == AOS else (lambda x: x.t().contiguous())
        for kind, x3 in (("rnea", tqdd), ("aba", ttau)):
            args = (put(tq), put(tqd), put(x3), put(tpi), GRAVITY, None, layout)
            fn = lambda m: m.rnea_parameters if kind == "rnea" else m.aba_parameters
            ref = fn(hm)(*args)
            torch.cuda.synchronize()
            view = hm.context()
            view.reserve(B)
            out = torch.empty_like(ref)
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            with torch.cuda.stream(s1):
                assert fn(view)(*args, out=out) is out  # the context's first call
                view.check(s1.cuda_stream)
                assert torch.equal(out, ref)
                out.zero_()
            torch.cuda.synchronize()
            with torch.cuda.stream(s2):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s2):
                    fn(view)(*args, out=out)
            torch.cuda.synchronize()
            assert not out.any()  # captured, not executed
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
            view.close()


def test_refusals_leave_the_output_untouched(torch_cuda):
    from mecano_amd import _lib
    torch = torch_cuda
    sys_, desc = make_case("arm7")
    hm, B, nv, n = model_of(desc), 10, desc.nv, desc.n_joints
    lib = _lib.load()
    q, qd, qdd, tau, pi = (dev(torch, x) for x in batch(sys_, desc, B))
    pi = pi.reshape(B, -1).contiguous()
    out, guard = poisoned(torch, B, (nv,), torch.float64)
    opts = hm._options(AOS, stream=torch.cuda.current_stream().cuda_stream)
    g3 = (ctypes.c_double * 3)(*GRAVITY)
    p = lambda x: x.data_ptr()
    for fn in (lib.mh_rnea_parameters_f64, lib.mh_aba_parameters_f64):
        assert fn(hm._h, B, p(q), p(qd), p(qdd), None, g3, None, ctypes.byref(opts), p(out)) == 1       # NULL pi
        assert fn(hm._h, B, None, p(qd), p(qdd), p(pi), g3, None, ctypes.byref(opts), p(out)) == 1      # NULL state
        assert fn(hm._h, B, p(q), p(qd), p(qdd), p(pi), None, None, ctypes.byref(opts), p(out)) == 1    # no gravity, no root acceleration
        assert fn(hm._h, -1, p(q), p(qd), p(qdd), p(pi), g3, None, ctypes.byref(opts), p(out)) == 2     # MH_ERR_BAD_DIMENSION
        assert fn(hm._h, 0, None, None, None, p(pi), g3, None, ctypes.byref(opts), p(out)) == 0         # B = 0: MH_OK, nothing touched
    with pytest.raises(_lib.MecanoHipError):  # wrong shapes
        hm.rnea_parameters(q, qd, qdd, pi[:, :-10].contiguous(), GRAVITY, out=out)
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_parameters(q, qd, tau, pi[:-1].contiguous(), GRAVITY, out=out)
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_parameters(q, qd, tau, pi, GRAVITY, out=torch.empty(B, nv + 1, dtype=torch.float64, device="cuda"))
    check_bad_outputs(torch, (B, nv), lambda o: hm.rnea_parameters(q, qd, qdd, pi, GRAVITY, out=o))
    check_bad_outputs(torch, (B, nv), lambda o: hm.aba_parameters(q, qd, tau, pi, GRAVITY, out=o))
    modes = [0] * n
    modes[3] = 1
    hm.set_joint_source_modes(modes)
    assert lib.mh_aba_parameters_f64(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, ctypes.byref(opts), p(out)) == 1  # acceleration sources
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_parameters(q, qd, tau, pi, GRAVITY, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(guard).all()
    assert lib.mh_rnea_parameters_f64(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, ctypes.byref(opts), p(out)) == 0  # the modes play no part
    hm.set_joint_source_modes(None)
    torch.cuda.synchronize()
    assert torch.equal(out, hm.rnea_parameters(q, qd, qdd, pi, GRAVITY))


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_a_massless_row_is_not_finite_alone(torch_cuda, layout):
    """One row with zero mass everywhere (no physical inertia): inf / nan in that row only, MH_OK; the other rows keep their bits."""
    torch = torch_cuda
    sys_, desc = make_case("humanoid30")
    hm, B, k = model_of(desc), 130, 64
    q, qd, qdd, tau, pi = batch(sys_, desc, B)
    good = run(torch, hm, "aba", q, qd, tau, pi, layout)
    bad = pi.copy()
    bad[k] = 0.0
    got = run(torch, hm, "aba", q, qd, tau, bad, layout)  # (raises on anything but MH_OK)
    keep = np.arange(B) != k
    assert not np.isfinite(got[k]).all()
    assert np.isfinite(got[keep]).all() and np.array_equal(got[keep], good[keep])


def test_numpy_round_trip(torch_cuda):
    sys_, desc = make_case("arm7")
    hm, ck = model_of(desc), ipc.Checker(desc)
    q, qd, qdd, tau, pi = batch(sys_, desc, 5)
    got = hm.rnea_parameters(q, qd, qdd, pi, GRAVITY)
    assert isinstance(got, np.ndarray) and got.shape == (5, desc.nv)
    close(got, ck.rnea(q, qd, qdd, pi, GRAVITY), 1e-10, label="numpy in, numpy out")
