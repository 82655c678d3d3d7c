"""The fp32 forms of the wider entry points -- mh_centroidal_f32, mh_crba_coriolis_f32, mh_rnea_bodies_f32, mh_aba_bodies_f32,
mh_aba_locked_f32, mh_integrate_f32 -- against the fp64 CPU checker (oracle.cpu_oracle.OracleModel) at the rounding-level bounds of
tests/helpers.py.  They are <float> instantiations of kernels whose fp64 form is well tested, and on a model with a code object they take
another plan than fp64 does, so a mistake in the fp32 form alone needs tests of its own.

Convention of every comparison: the states are rounded to fp32 first, the checker runs in fp64 on the rounded values, the device result is
widened to fp64, and the check goes through helpers.close / close_aba / record_parity (achieved error and bound land in the parity log).
Gravity, the time step and the centroidal frame are numbers fp32 holds exactly; the model's own parameters are rounded by the engine, as in
the fp32 tests of the core calls.  The Coriolis and the centroidal momentum matrices are sums along tree paths of at most n bodies like the
mass matrix, the integrator is one step per joint without recursion: f32_forward_tol(n) and f32_forward_tol(1).

Models (fixed seeds): the 30-DoF humanoid (it has a code object, which fp32 must not depend on: every result is bit for bit the one under
MH_DISABLE_SPEC=1), a 7-joint revolute chain (no tree split: the one-wave sweep kernels), a 12-joint tree with every joint kind.
B = 1, 65, 257 (a ragged wave, one wave and one lane, several waves), prefixes of one batch of 257 states whose references are computed
once.  The seeds are chosen so that the conditioning-scaled forward bounds of forward dynamics stay meaningful on at least three quarters
of the rows (test_forward_dynamics_bounds_of_the_chosen_seeds_bind, which needs no device).

This file holds two tests that need no device beside the device ones, so the gpu mark is set per test, not on the module."""
import functools
import types

import numpy as np
import pytest

import helpers
from helpers import U32, close, close_aba, f32_aba_backward_tol, f32_aba_forward_factor, f32_forward_tol

gpu = pytest.mark.gpu

ALL_KINDS = ("revolute", "prismatic", "planar", "spherical", "sixdof", "fixed")
MODELS = ("humanoid", "chain7", "kinds12")
LOCKED_MODELS = ("humanoid", "kinds12")
MODEL_SEEDS = {"humanoid": 43, "chain7": 7, "kinds12": 43}
STATE_SEEDS = {"humanoid": 2342, "chain7": 70, "kinds12": 120}
BATCHES = (1, 65, 257)
BMAX = max(BATCHES)
G = (0.25, -0.5, -9.8125)  # exact in fp32
DT = 2.0 ** -9  # exact in fp32, and so is dt^2 / 2
NDOF = {0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}  # revolute, prismatic, sixdof, fixed, planar, spherical (mecano_amd.multibody)
NCFG = {0: 1, 1: 1, 2: 7, 3: 0, 4: 3, 5: 4}
SIXDOF, PLANAR, SPHERICAL = 2, 4, 5


def r32(x):
    """x rounded to fp32, held in fp64, read-only: what the device gets and what the checker gets"""
    a = np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
    a.setflags(write=False)
    return a


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(name):
    """Model, checker and the one batch of fp32-rounded states of a model; everything in it is shared between the tests and read-only."""
    from mecano_amd import random_tools as rt
    from mecano_amd.multibody import MultiBodySystem
    from oracle.cpu_oracle import OracleModel
    rng = np.random.default_rng(MODEL_SEEDS[name])
    if name == "humanoid":
        sys_ = rt.nextHumanoid(rng)
    else:
        joints = rt.nextJointChain(rng, 7, ("revolute",)) if name == "chain7" else rt.nextJointTree(rng, 12, ALL_KINDS)
        sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
    d = sys_.toModelDesc()
    rng = np.random.default_rng(STATE_SEEDS[name])
    q, qd, qdd, tau = (r32(x) for x in rt.nextState(rng, sys_, BMAX))
    fext = r32(rng.uniform(-1, 1, (BMAX, d.n_joints, 6)))
    Rf = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    Rf *= np.sign(np.linalg.det(Rf))
    frame = r32(np.concatenate([Rf.ravel(), rng.uniform(-1, 1, 3)]))
    ofs = np.concatenate([[0], np.cumsum([NDOF[int(t)] for t in d.joint_type])])
    joint_dofs = [np.asarray(d.dof_indices[ofs[j]:ofs[j + 1]], dtype=np.int64) for j in range(d.n_joints)]
    ofs = np.concatenate([[0], np.cumsum([NCFG[int(t)] for t in d.joint_type])])
    joint_cfgs = [np.asarray(d.cfg_indices[ofs[j]:ofs[j + 1]], dtype=np.int64) for j in range(d.n_joints)]
    return types.SimpleNamespace(name=name, sys=sys_, d=d, om=OracleModel(d), n=d.n_joints, nv=d.nv, nq=d.nq, q=q, qd=qd, qdd=qdd, tau=tau,
                                 fext=fext, frame=frame, joint_dofs=joint_dofs, joint_cfgs=joint_cfgs)


CENTROIDAL_MODES = ("root frame, fixed", "random frame, at the centre of mass")


@functools.lru_cache(maxsize=None)
def centroidal_ref(name, mode):
    c = case(name)
    frame, at_com = (None, False) if mode == CENTROIDAL_MODES[0] else (c.frame, True)
    return frozen(*c.om.centroidal(c.q, c.qd, frame, at_com))


@functools.lru_cache(maxsize=None)
def coriolis_ref(name):
    """(H, C, the bias RNEA(q, qd, 0) without gravity)"""
    c = case(name)
    H, C = c.om.crba_coriolis(c.q, c.qd)
    return frozen(H, C, c.om.rnea(c.q, c.qd, np.zeros_like(c.qd), (0.0, 0.0, 0.0)))


def cond_inf(H):
    """cond_inf of every matrix of a stack; 1 for the empty system"""
    return np.linalg.cond(H, np.inf) if H.shape[-1] else np.ones(H.shape[0])


@functools.lru_cache(maxsize=None)
def conds_of(name):
    return frozen(cond_inf(coriolis_ref(name)[0]))[0]


def fext_of(c, with_f):
    return c.fext if with_f else None


@functools.lru_cache(maxsize=None)
def rnea_bodies_ref(name, with_f):
    c = case(name)
    return frozen(*c.om.rnea_bodies(c.q, c.qd, c.qdd, G, fext_of(c, with_f)))


@functools.lru_cache(maxsize=None)
def aba_bodies_ref(name, with_f):
    """(qdd, body accelerations, body twists, the bias RNEA(q, qd, 0))"""
    c = case(name)
    f = fext_of(c, with_f)
    return frozen(*c.om.aba_bodies(c.q, c.qd, c.tau, G, f), c.om.rnea(c.q, c.qd, np.zeros_like(c.qd), G, f))


LOCK_PATTERNS = ("every third joint", "all joints", "no joint")


def locked_flags(c, pattern):
    """(one flag per joint, True for the DoFs of the locked joints)"""
    flags = {"every third joint": np.arange(c.n) % 3 == 0, "all joints": np.ones(c.n, bool), "no joint": np.zeros(c.n, bool)}[pattern]
    dofs = np.zeros(c.nv, dtype=bool)
    for j in np.flatnonzero(flags):
        dofs[c.joint_dofs[j]] = True
    return flags.astype(np.int32), dofs


@functools.lru_cache(maxsize=None)
def locked_conds(name, pattern):
    """cond_inf of H restricted to the unlocked DoFs: the system forward dynamics solves with the other joints on given accelerations"""
    c = case(name)
    free = np.flatnonzero(~locked_flags(c, pattern)[1])
    return frozen(cond_inf(coriolis_ref(name)[0][:, free][:, :, free]))[0]


@functools.lru_cache(maxsize=None)
def locked_ref(name, pattern, with_f):
    c = case(name)
    return frozen(*c.om.aba_locked(c.q, c.qd, c.tau, c.qdd, locked_flags(c, pattern)[0], G, fext_of(c, with_f)))


# ---- the integrator's rows with a chosen rotation step.  rv = dt w + dt^2 / 2 alpha is the rotation vector of the 6-DoF and spherical
# joints; below |rv| = 1e-12 both the engine and the checker take the identity.  (row, |rv|) and (row, pitch step of the planar joints):
ROTATION_ROWS = ((0, 0.0), (1, 0.5e-12), (2, 2.0e-12), (3, np.pi), (4, 2.0 * np.pi + 0.3), (64, np.pi), (256, 2.0 * np.pi + 0.3))
PITCH_ROWS = ((5, 0.0), (6, 7.0))
SPECIAL_ROWS = tuple(r for r, _ in ROTATION_ROWS + PITCH_ROWS)
IDENTITY_ROWS = (0, 1)  # |rv| = 0 and |rv| below the threshold: dq is the identity and q * dq is q, bit for bit


@functools.lru_cache(maxsize=None)
def integrator_case(name):
    """(q, qd, qdd) of case(name) with the special rows overwritten, fp32-rounded, and the checker's step of them."""
    c = case(name)
    q, qd, qdd = c.q.copy(), c.qd.copy(), c.qdd.copy()
    rng = np.random.default_rng(STATE_SEEDS[name] + 1)
    hdd = 0.5 * DT * DT
    for j in range(c.n):
        t, dofs = int(c.d.joint_type[j]), c.joint_dofs[j]
        if t in (SIXDOF, SPHERICAL):
            ang = dofs[:3]
            for row, mag in ROTATION_ROWS:
                u = rng.normal(size=3)
                u /= np.linalg.norm(u)
                if mag < 1.0:  # zero (the linear velocity of a 6-DoF joint stays as drawn), or next to the threshold: no acceleration
                    qdd[row, ang] = 0.0
                qd[row, ang] = (mag * u - hdd * qdd[row, ang]) / DT
        elif t == PLANAR:
            for row, step in PITCH_ROWS:
                qd[row, dofs[0]], qdd[row, dofs[0]] = step / DT, 0.0
    q, qd, qdd = r32(q), r32(qd), r32(qdd)
    for j in range(c.n):  # the rounded rows still are where they were put
        if int(c.d.joint_type[j]) in (SIXDOF, SPHERICAL):
            ang = c.joint_dofs[j][:3]
            for row, mag in ROTATION_ROWS:
                th = np.linalg.norm(DT * qd[row, ang] + hdd * qdd[row, ang])
                assert th == 0.0 if mag == 0.0 else abs(th - mag) <= 1e-6 * mag, (row, mag, th)
    return (q, qd, qdd) + frozen(*c.om.integrate(DT, q, qd, qdd))


# ---------------------------------------------------------------------------------------------------- the comparisons
def check_centroidal(got, ref, n, label=""):
    """A and com entry by entry; b on the scale max(1, |A|_inf, |b|_inf) (its terms are A's entries times velocities)"""
    (A, b, com), (rA, rb, rcom) = got, ref
    tol = f32_forward_tol(n)
    close(A, rA, tol, label=label + "A")
    close(com, rcom, tol, label=label + "com")
    if b is not None:
        err, bound = float(np.abs(b - rb).max()), tol * max(1.0, float(np.abs(rA).max(initial=0.0)), float(np.abs(rb).max()))
        helpers.record_parity(err, bound, label + "b")
        assert err <= bound, f"b: max err {err:.3e} > {bound:.3e}"


def check_product(M, M_ref, qd, ref, n, label):
    """M qd in fp64 host arithmetic against `ref`, row by row within f32_forward_tol(n) |M_ref|_inf ||qd||_1: every entry of M is within
    f32_forward_tol(n) max(1, |M_ref|_inf) of M_ref, and a row of the product sums nv of them weighted by |qd|."""
    got = np.einsum("bij,bj->bi", M, qd)
    bound = f32_forward_tol(n) * float(np.abs(M_ref).max()) * np.abs(qd).sum(axis=1)
    ratio = float((np.abs(got - ref).max(axis=1) / bound).max())
    helpers.record_parity(ratio, 1.0, label + " / (tol |M|_inf |qd|_1)")
    assert ratio <= 1.0, f"{label}: err / bound = {ratio:.3e}"


def check_coriolis(H, C, H_ref, C_ref, n, label=""):
    tol = f32_forward_tol(n)
    close(H, H_ref, tol, label=label + "H")
    close(C, C_ref, tol, label=label + "C")
    assert np.array_equal(H == 0, H_ref == 0), "H: zeros of unrelated joints"


def check_rnea_bodies(got, ref, n, label=""):
    for x, r, what in zip(got, ref, ("tau", "body acc", "body twist")):
        close(x, r, f32_forward_tol(n), label=label + what)


def check_aba_bodies(got, ref, conds, n, label=""):
    """qdd and the body accelerations (sums of S qdd along the paths) row by row on the conditioning of the row's H; the twists do not
    depend on the solve"""
    B = len(conds)
    for x, r, what in zip(got[:2], ref[:2], ("qdd", "body acc")):
        close_aba(x.reshape(B, -1), r.reshape(B, -1), None, n, u=U32, label=label + what, conds=conds)
    close(got[2], ref[2], f32_forward_tol(n), label=label + "body twist")


def check_backward_error(om, q, qd, qdd32, tau, bias, f, n, label):
    """|RNEA_fp64(q, qd, qdd32) - tau|_inf <= f32_aba_backward_tol(n) (|tau|_inf + |bias|_inf), each row on its own scale: the rows are
    independent problems, and this holds whatever the conditioning"""
    err = np.abs(om.rnea(q, qd, qdd32, G, f) - tau).max(axis=1)
    ratio = float((err / (np.abs(tau).max(axis=1) + np.abs(bias).max(axis=1))).max())
    helpers.record_parity(ratio, f32_aba_backward_tol(n), label)
    assert ratio <= f32_aba_backward_tol(n), f"{label}: {ratio:.3e} > {f32_aba_backward_tol(n):.3e}"


def binding_share(conds, n):
    """share of the rows on which the forward bound of forward dynamics is at most 1e-2"""
    return float(np.mean(f32_aba_forward_factor(n) * conds * U32 <= 1.0e-2))


# ---------------------------------------------------------------------------------------------------- without a device
def test_forward_dynamics_bounds_of_the_chosen_seeds_bind():
    """close_aba's bound grows with cond_inf(H) of the row: on an ill-conditioned batch it would let anything pass.  Checker only: for
    every forward-dynamics case below (every model, every B; the locked patterns with H of the unlocked DoFs) at least three quarters of
    the rows have f32_aba_forward_factor(n) cond U32 <= 1e-2.  (The backward error covers every row regardless.)"""
    for name in MODELS:
        c = case(name)
        for B in BATCHES:
            share = binding_share(conds_of(name)[:B], c.n)
            assert share >= 0.75, (name, B, share)
    for name in LOCKED_MODELS:
        c = case(name)
        for pattern in LOCK_PATTERNS:
            for B in BATCHES:
                share = binding_share(locked_conds(name, pattern)[:B], c.n)
                assert share >= 0.75, (name, pattern, B, share)


def test_bounds_reject_a_relative_error_of_1e_4(monkeypatch):
    """The comparisons have teeth: the checker's own C, centroidal A and body accelerations of the humanoid, scaled by 1 + 1e-4 -- twenty
    times inside the flat 2e-3 that guarded the Coriolis matrix before -- are rejected; unscaled they pass."""
    monkeypatch.setattr(helpers, "record_parity", lambda *a, **k: None)  # synthetic outputs stay out of the parity log
    c, s = case("humanoid"), 1.0 + 1.0e-4
    H, C, bias = coriolis_ref("humanoid")
    check_coriolis(H, C, H, C, c.n)
    check_product(C, C, c.qd, bias, c.n, "C qd")
    with pytest.raises(AssertionError):
        check_coriolis(H, C * s, H, C, c.n)
    for mode in CENTROIDAL_MODES:
        A, b, com = centroidal_ref("humanoid", mode)
        check_centroidal((A, b, com), (A, b, com), c.n)
        with pytest.raises(AssertionError):
            check_centroidal((A * s, b, com), (A, b, com), c.n)
    for with_f in (False, True):
        tau, acc, tw = rnea_bodies_ref("humanoid", with_f)
        check_rnea_bodies((tau, acc, tw), (tau, acc, tw), c.n)
        with pytest.raises(AssertionError):
            check_rnea_bodies((tau, acc * s, tw), (tau, acc, tw), c.n)


# ---------------------------------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def put(torch, x, B, soa, dtype=None):
    """rows 0 .. B-1 of a host array as a device matrix of the layout: [B, k] or [k, B]"""
    if x is None:
        return None
    t = torch.tensor(np.ascontiguousarray(x[:B]).reshape(B, -1), device="cuda", dtype=dtype or torch.float32)
    return t.t().contiguous() if soa else t


def get(t, soa, shape):
    """a device output as a host array of `shape` = (B, ...), in its own dtype"""
    if t is None:
        return None
    a = t.cpu().numpy()
    return np.ascontiguousarray(a.T if soa else a).reshape(shape)


def wide(xs):
    return tuple(None if x is None else x.astype(np.float64) for x in xs)


def layout_of(soa):
    from mecano_amd import _lib
    return _lib.LAYOUT_SOA if soa else _lib.LAYOUT_AOS


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def without_code_object(monkeypatch, d):
    """the model built with the topology-specialised code object switched off"""
    from mecano_amd.engine import HipModel
    monkeypatch.setenv("MH_DISABLE_SPEC", "1")
    hm = HipModel(d)
    monkeypatch.delenv("MH_DISABLE_SPEC")
    return hm


def run_centroidal(torch, hm, c, B, mode, soa, with_qd=True):
    frame, at_com = (None, False) if mode == CENTROIDAL_MODES[0] else (c.frame, True)
    A, b, com = hm.centroidal(put(torch, c.q, B, soa), put(torch, c.qd, B, soa) if with_qd else None, frame, at_com, layout_of(soa))
    return get(A, soa, (B, 6, c.nv)), get(b, soa, (B, 6)), get(com, soa, (B, 3))


@gpu
@pytest.mark.parametrize("name", MODELS)
def test_centroidal_momentum_fp32(torch_cuda, monkeypatch, name):
    """mh_centroidal_f32 with data: A, b and the frame origin for the root frame and for a random frame at the centre of mass, with and
    without qd (no b then), SoA bit-equal to AoS, and A32 qd against the checker's momentum A qd."""
    from mecano_amd.engine import HipModel
    torch, c = torch_cuda, case(name)
    hm = HipModel(c.d)
    plain = without_code_object(monkeypatch, c.d) if name == "humanoid" else None
    for B in BATCHES:
        for mode in CENTROIDAL_MODES:
            ref = tuple(x[:B] for x in centroidal_ref(name, mode))
            got = run_centroidal(torch, hm, c, B, mode, False)
            assert got[0].dtype == np.float32 and not any(np.isnan(x).any() for x in got)
            check_centroidal(wide(got), ref, c.n)
            check_product(got[0].astype(np.float64), ref[0], c.qd[:B], np.einsum("bij,bj->bi", ref[0], c.qd[:B]), c.n, "A qd")
            assert same(run_centroidal(torch, hm, c, B, mode, True), got), "SoA differs from AoS"
            for soa in (False, True):
                A_only, b_none, com_only = run_centroidal(torch, hm, c, B, mode, soa, with_qd=False)
                assert b_none is None
                check_centroidal(wide((A_only, None, com_only)), ref, c.n, label="without qd: ")
            if plain is not None:
                assert same(run_centroidal(torch, plain, c, B, mode, False), got), "fp32 depends on the code object"


def run_coriolis(torch, hm, c, B, soa):
    H, C = hm.crba_coriolis(put(torch, c.q, B, soa), put(torch, c.qd, B, soa), layout_of(soa))
    return get(H, soa, (B, c.nv, c.nv)), get(C, soa, (B, c.nv, c.nv))


@gpu
@pytest.mark.parametrize("name", MODELS)
def test_mass_and_coriolis_matrix_fp32(torch_cuda, monkeypatch, name):
    """mh_crba_coriolis_f32: H and C entry by entry, exact zeros of H, SoA bit-equal to AoS, and the reference's invariant C qd =
    RNEA(q, qd, 0) without gravity with the checker's bias on the right."""
    from mecano_amd.engine import HipModel
    torch, c = torch_cuda, case(name)
    hm = HipModel(c.d)
    plain = without_code_object(monkeypatch, c.d) if name == "humanoid" else None
    for B in BATCHES:
        H_ref, C_ref, bias = (x[:B] for x in coriolis_ref(name))
        got = run_coriolis(torch, hm, c, B, False)
        assert got[1].dtype == np.float32 and not any(np.isnan(x).any() for x in got)
        H, C = wide(got)
        check_coriolis(H, C, H_ref, C_ref, c.n)
        check_product(C, C_ref, c.qd[:B], bias, c.n, "C qd")
        assert same(run_coriolis(torch, hm, c, B, True), got), "SoA differs from AoS"
        if plain is not None:
            assert same(run_coriolis(torch, plain, c, B, False), got), "fp32 depends on the code object"


@gpu
@pytest.mark.parametrize("name", MODELS)
def test_per_body_outputs_fp32_on_both_plans(torch_cuda, monkeypatch, name):
    """mh_rnea_bodies_f32 / mh_aba_bodies_f32 on the run-time tree split (MH_SPLIT_RT=1) and on the one-wave sweep kernels (MH_SPLIT_RT=0),
    both without a code object, and on the humanoid as built by default (which must give one of the two, bit for bit): all three outputs of
    each call against the checker, forward dynamics also by its backward error on every row; with and without external wrenches, both
    layouts."""
    from mecano_amd.engine import HipModel
    torch, c = torch_cuda, case(name)
    builds = {}
    monkeypatch.setenv("MH_DISABLE_SPEC", "1")
    for plan, flag in (("split", "1"), ("sweep", "0")):
        monkeypatch.setenv("MH_SPLIT_RT", flag)
        builds[plan] = HipModel(c.d)
    monkeypatch.delenv("MH_DISABLE_SPEC")
    monkeypatch.delenv("MH_SPLIT_RT")
    assert "run-time tree split" not in builds["sweep"].kernel_variant
    assert ("run-time tree split" in builds["split"].kernel_variant) == (name != "chain7"), builds["split"].kernel_variant
    if name == "humanoid":
        builds["default"] = HipModel(c.d)
    for with_f in (False, True):
        f = fext_of(c, with_f)
        for B in BATCHES:
            r_ref = tuple(x[:B] for x in rnea_bodies_ref(name, with_f))
            a_ref = tuple(x[:B] for x in aba_bodies_ref(name, with_f))
            shapes = ((B, c.nv), (B, c.n, 6), (B, c.n, 6))
            for soa in (False, True):
                q, qd, qdd, tau, tf = (put(torch, x, B, soa) for x in (c.q, c.qd, c.qdd, c.tau, f))
                if tf is not None and not soa:
                    tf = tf.reshape(B, c.n, 6)
                results = {}
                for plan, hm in builds.items():
                    label = plan + ": "
                    r = tuple(get(x, soa, s) for x, s in zip(hm.rnea_bodies(q, qd, qdd, G, tf, layout_of(soa)), shapes))
                    a = tuple(get(x, soa, s) for x, s in zip(hm.aba_bodies(q, qd, tau, G, tf, layout_of(soa)), shapes))
                    assert all(x.dtype == np.float32 and not np.isnan(x).any() for x in r + a)
                    check_rnea_bodies(wide(r), r_ref, c.n, label + "rnea_bodies ")
                    check_aba_bodies(wide(a), a_ref, conds_of(name)[:B], c.n, label + "aba_bodies ")
                    check_backward_error(c.om, c.q[:B], c.qd[:B], a[0].astype(np.float64), c.tau[:B], a_ref[3], None if f is None else f[:B], c.n,
                                         label + "aba_bodies backward error / (|tau| + |bias|)")
                    results[plan] = r + a
                if "default" in results:
                    assert same(results["default"], results["split"]) or same(results["default"], results["sweep"]), \
                        "fp32 per-body outputs depend on the code object"


@gpu
@pytest.mark.parametrize("name", LOCKED_MODELS)
def test_locked_joints_fp32(torch_cuda, monkeypatch, name):
    """mh_aba_locked_f32 with every third joint, every joint and no joint on a given acceleration: the given accelerations and the given
    efforts come back bit for bit, (qdd, tau) against the checker on the conditioning of H restricted to the unlocked DoFs (the system
    that is solved), and with every joint locked tau is inverse dynamics."""
    from mecano_amd.engine import HipModel
    torch, c = torch_cuda, case(name)
    hm = HipModel(c.d)
    plain = without_code_object(monkeypatch, c.d) if name == "humanoid" else None
    rnea_ref = {}
    for pattern in LOCK_PATTERNS:
        flags, lock_dofs = locked_flags(c, pattern)
        conds = locked_conds(name, pattern)
        for with_f in (False, True):
            f = fext_of(c, with_f)
            ref = locked_ref(name, pattern, with_f)
            for B in BATCHES:
                for soa in (False, True):
                    q, qd, tau, qdd, tf = (put(torch, x, B, soa) for x in (c.q, c.qd, c.tau, c.qdd, f))
                    if tf is not None and not soa:
                        tf = tf.reshape(B, c.n, 6)
                    hm.set_joint_source_modes(flags)
                    got = tuple(get(x, soa, (B, c.nv)) for x in hm.aba_locked(q, qd, tau, qdd, G, tf, layout_of(soa)))
                    hm.set_joint_source_modes(None)
                    assert all(x.dtype == np.float32 and not np.isnan(x).any() for x in got)
                    a, t = wide(got)
                    assert np.array_equal(a[:, lock_dofs], c.qdd[:B, lock_dofs]), "the given accelerations come back changed"
                    assert np.array_equal(t[:, ~lock_dofs], c.tau[:B, ~lock_dofs]), "the given efforts come back changed"
                    close_aba(a, ref[0][:B], None, c.n, u=U32, label=pattern + ": qdd", conds=conds[:B])
                    close_aba(t, ref[1][:B], None, c.n, u=U32, label=pattern + ": tau", conds=conds[:B])
                    if pattern == "all joints":
                        if with_f not in rnea_ref:
                            rnea_ref[with_f] = c.om.rnea(c.q, c.qd, c.qdd, G, f)
                        close(t, rnea_ref[with_f][:B], f32_forward_tol(c.n), label="all joints: tau against inverse dynamics")
                    if plain is not None and not soa:
                        plain.set_joint_source_modes(flags)
                        other = tuple(get(x, soa, (B, c.nv)) for x in plain.aba_locked(q, qd, tau, qdd, G, tf))
                        plain.set_joint_source_modes(None)
                        assert same(other, got), "fp32 depends on the code object"


def run_integrate(torch, hm, state, B, soa, dtype, with_acc):
    q, qd, qdd = (put(torch, x, B, soa, dtype) for x in state)
    out = hm.integrate(DT, q, qd, qdd, layout_of(soa), return_acceleration=with_acc)
    return tuple(get(x, soa, (B, -1)) for x in out)


@gpu
@pytest.mark.parametrize("name", LOCKED_MODELS)
def test_state_integrator_fp32_and_the_small_angle_branch(torch_cuda, monkeypatch, name):
    """mh_integrate_f32 at f32_forward_tol(1) -- the step is per joint, nothing is summed along the tree --, and in both precisions the
    rows the random states never reach: the rotation vector of the 6-DoF and spherical joints exactly zero, on either side of the 1e-12
    below which the engine and the checker both take the identity, at pi and beyond 2 pi; a planar pitch step of 0 and of 7.  fp64 keeps
    the bounds it has on random rows (1e-13 on the state, 1e-12 on the re-expressed acceleration).  Every special row is compared on its
    own scale (its velocities reach thousands), the ordinary rows together.  No NaN; a rotation vector of zero, or below the threshold, leaves the quaternion
    bit for bit; the state is the same with and without the acceleration output; both layouts."""
    from mecano_amd.engine import HipModel
    torch, c = torch_cuda, case(name)
    hm = HipModel(c.d)
    plain = without_code_object(monkeypatch, c.d) if name == "humanoid" else None
    q, qd, qdd, rq, rv, ra = integrator_case(name)
    quat = np.concatenate([c.joint_cfgs[j][:4] for j in range(c.n) if int(c.d.joint_type[j]) in (SIXDOF, SPHERICAL)])
    for dtype, tols in ((torch.float32, (f32_forward_tol(1),) * 3), (torch.float64, (1e-13, 1e-13, 1e-12))):
        tag = "fp32 " if dtype == torch.float32 else "fp64 "
        for B in BATCHES:
            special = [r for r in SPECIAL_ROWS if r < B]
            ordinary = np.setdiff1d(np.arange(B), special)
            for soa in (False, True):
                got = run_integrate(torch, hm, (q, qd, qdd), B, soa, dtype, True)
                assert not any(np.isnan(x).any() for x in got)
                g64 = wide(got)
                for x, r, tol, what in zip(g64, (rq, rv, ra), tols, ("q", "qd", "qdd")):
                    if len(ordinary):
                        close(x[ordinary], r[ordinary], tol, label=tag + what)
                    for row in special:
                        close(x[row], r[row], tol, label=tag + what + ", special rows")
                for row in (r for r in IDENTITY_ROWS if r < B):
                    assert np.array_equal(g64[0][row, quat], q[row, quat]), "a rotation vector below the threshold changed the quaternion"
                assert same(run_integrate(torch, hm, (q, qd, qdd), B, soa, dtype, False), got[:2]), "the state depends on the acceleration output"
                if plain is not None and dtype == torch.float32 and not soa:
                    assert same(run_integrate(torch, plain, (q, qd, qdd), B, soa, dtype, True), got), "fp32 depends on the code object"
