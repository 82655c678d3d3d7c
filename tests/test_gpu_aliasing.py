"""The aliasing contract of the compute calls (include/mecano_hip.h, "Aliasing"), on every kernel plan the dispatcher can take.

An ALLOWED aliasing is held to one criterion: on one model, one batch size, one layout and one stream the call runs once out of place into
a poisoned buffer with a guard row and once aliased on fresh copies of the inputs; the aliased result is bit for bit the out-of-place one
(torch.equal, no tolerance) and every other input of the aliased call is unchanged.  The out-of-place results of these plans are held to
the oracle by tests/test_gpu_persistent_loops.py.  A FORBIDDEN overlap returns MH_ERR_INVALID_ARGUMENT with "overlap" in mh_last_error,
writes nothing, and the next valid call on the model is right.

Plans and the dispatcher conditions that select them (mecano_amd/csrc/mh_api.hip: zv_ok, zvf_ok, zvb_ok, rnea_ahead_ok, split_ok, launch<T>;
cu = MH_FAKE_CU_COUNT where given, groups = ceil(B / 64)).  Every plan runs at B = 357 with cu = 1 (six groups on a grid of two or
fewer workgroups: three turns or more, a ragged last group), at B = 129 with cu = 3, and at B = 1 and 64 on the real device, unless
its row names other sizes; the parameter, locked, per-body, pair and integrator calls (run-time kernels, one plan each) run at 357, 64
and 1 as their tests list them.

Humanoid, fp64, AoS, mh_aba_f64, qdd_out = tau and qdd_out = qd:
  bias_split    MH_ZV=2                         zv_ok: use_zv == 2 takes the two-job launch at every batch size
  fused         MH_ZV=0 MH_ZVF=2                zv_ok false (use_zv = 0); zvf_ok: use_zvf == 2 (default: groups > cu)
  two_launch    MH_ZV=0 MH_ZVF=0 MH_ZVB=2       zvf_ok false; zvb_ok: use_zvb == 2 (default: groups >= 2 cu)
  tree_split    MH_ZV=0 MH_ZVF=0 MH_ZVB=0       split_ok (algo 1: always); rows staged in LDS (split_flags: SPEC_IO_LDS), grid min(groups, 2 cu)
  tree_split_direct   ... MH_SPEC_IO=0          force_io == 0: zv / zvf / zvb refuse, split_flags without SPEC_IO_LDS -- rows read directly
  whole_tree    MH_SPEC_SPLIT=0 (MH_SPEC_ST=0|1)   use_split == 0: no tree-split plan; model->spec.launch with SPEC_ST_LDS by force_st.  The
                                                humanoid's code object carries the whole-tree inverse dynamics only (mh_spec.hip: kWholeTreeAba
                                                needs a tree without a split form): its forward dynamics goes on to the run-time kernels
  run_time_split   MH_DISABLE_SPEC=1 MH_SPLIT_RT=1   use_spec = 0; split_rt.usable && use_split_rt == 1: launch_split_rt at every size
  sweep         MH_DISABLE_SPEC=1 MH_SPLIT_RT=0    fp64 forward dynamics stays on aba_kernel (dfs_aba false), fp64 RNEA on the depth-first walk
  depth_first   ... MH_DFS_ABA64=1              dfs_aba64: launch_dfs for fp64 forward dynamics too
Humanoid, fp64, mh_rnea_f64, tau_out = qdd and tau_out = qd:
  ahead         MH_RNEA_AHEAD=2                 rnea_ahead_ok: use_rnea_ahead == 2 (default: groups > 2 cu)
  tree_split    MH_RNEA_AHEAD=0                 split_ok (algo 0: always), AoS rows in LDS; with SoA matrices: rnea_ahead_ok and SPEC_IO_LDS are
                                                off for SoA, rows read directly
  whole_tree, run_time_split, sweep (= depth-first RNEA; MH_DFS=0: rnea_kernel)   as above
The 128-body tree (no code object), fp32 and fp64, AoS and SoA, RNEA and ABA:
  depth_first   MH_FAKE_CU_COUNT=1, B = 357     groups > 2 cu: past the run-time tree split; use_dfs: launch_dfs (fp64 ABA: aba_kernel)
  transposed    MH_GENERIC_TRANSPOSE=1 MH_FAKE_CU_COUNT=3, B = 453   transposes(): AoS rows through scratch copies (ABA; RNEA keeps LDS row windows)
  sweep         MH_DFS=0 MH_FAKE_CU_COUNT=1     use_dfs = 0: rnea_kernel / aba_kernel
  run_time_split   B = 64 on the real device    groups <= 2 cu: launch_split_rt
arm7 (nq == nv, revolute joints, identity maps): the output as q, with its code object (whole-tree kernels) and with MH_DISABLE_SPEC=1.
A 14-joint branching revolute tree (no code object): the output as q on the run-time tree split (MH_SPLIT_RT=1: every size), the
depth-first walks (MH_SPLIT_RT=0) and the sweep kernels (MH_DFS=0).
A 12-joint revolute / prismatic tree with permuted dof_indices and cfg_indices: the non-identity-map plans, the output as the third input
(the output as q is refused there: prismatic coordinates are read from q again after the joint's output is stored)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from helpers import DistinctRows
from test_gpu_persistent_loops import DT, G, _out, prepare, robot, switches  # (_out: helpers.poisoned outputs with a guard row)

pytestmark = pytest.mark.gpu

MORE_KEYS = ("MH_GENERIC_TRANSPOSE", "MH_SPEC_IO", "MH_SPEC_ST", "MH_DFS", "MH_DFS_ABA64", "MH_ZV_STEP")
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@contextlib.contextmanager
def all_switches(**env):
    """switches() of test_gpu_persistent_loops clears and restores its KEYS only: the same for the switches this module sets besides."""
    saved = {k: os.environ.pop(k, None) for k in MORE_KEYS}
    try:
        with switches(**env):
            yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Case:
    """A robot that is not one of test_gpu_persistent_loops.robot(): description, distinct rows, and how its state columns are laid out."""

    def __init__(self, sys_, desc, perm=None):
        self.sys, self.d, self.perm = sys_, desc, perm
        self.rows = DistinctRows(sys_, 64, 77)

    def device(self, torch, B, dt):
        ins = self.rows.device(torch, B, dt)
        if self.perm is None:
            return ins
        idx = torch.as_tensor(self.perm.astype(np.int64), device="cuda")
        moved = []
        for x in ins:  # joint k owns column perm[k]
            y = torch.zeros_like(x)
            y[:, idx] = x
            moved.append(y)
        return tuple(moved)


_CASES, _MODELS = {}, {}


class Shared:
    """A robot of test_gpu_persistent_loops.robot() (built once for both modules), read only."""

    def __init__(self, rb):
        self.sys, self.d, self.rows = rb.sys, rb.d, rb.rows

    def device(self, torch, B, dt):
        return self.rows.device(torch, B, dt)


def case(name):
    if name not in _CASES:
        if name in ("humanoid", "tree128"):
            _CASES[name] = Shared(robot(name))
        elif name == "rev14":  # a branching tree of revolute joints, identity maps, no code object: the output may be q
            from mecano_amd import random_tools as rt
            from mecano_amd.multibody import MultiBodySystem
            joints = rt.nextJointTree(np.random.default_rng(14), 14, ("revolute",))
            sys_ = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
            _CASES[name] = Case(sys_, sys_.toModelDesc())
        elif name == "perm12":  # as tests/test_gpu_inertial_parameters.py::test_custom_index_provider_and_listing_order
            from mecano_amd import random_tools as rt
            from mecano_amd.multibody import MultiBodySystem
            rng = np.random.default_rng(31)
            sys_ = MultiBodySystem.toMultiBodySystemInput(rt.nextJointTree(rng, 12, ("revolute", "prismatic"))[0].getPredecessor())
            d = sys_.toModelDesc()
            perm = rng.permutation(d.nv).astype(np.int32)
            d.dof_indices, d.cfg_indices = perm.copy(), perm.copy()
            _CASES[name] = Case(sys_, d, perm)
        else:
            from test_inertial_parameters_cpu import make_case
            _CASES[name] = Case(*make_case(name))
    return _CASES[name]


def model(name, **env):
    """one model per (robot, switch set), shared by every aliasing and batch size"""
    key = (name, tuple(sorted(env.items())))
    if key not in _MODELS:
        from mecano_amd.engine import HipModel
        with all_switches(**env):
            _MODELS[key] = HipModel(case(name).d)
    return _MODELS[key]


# ---- binding an entry point to fresh copies of its inputs and poisoned outputs: (fn, [arguments], inputs as passed, [(rows, guard)], keep)
# the last len(outputs) arguments are the output pointers
STATE = {"rnea": (0, 1, 2), "aba": (0, 1, 3), "rnea_parameters": (0, 1, 2), "aba_parameters": (0, 1, 3), "aba_locked": (0, 1, 3, 2),
         "rnea_bodies": (0, 1, 2), "aba_bodies": (0, 1, 3), "rnea_joint_wrenches": (0, 1, 2), "aba_joint_wrenches": (0, 1, 3),
         "rnea_crba": (0, 1, 2), "integrate": (0, 1, 2), "aba_integrate": (0, 1, 3), "rnea_aba": (0, 1, 2, 3),
         "rnea_derivatives": (0, 1, 2), "aba_derivatives": (0, 1, 3)}


def out_shapes(hm, name):
    nv, nq, nj = hm.nv, hm.nq, hm.n_joints
    return {"rnea": [(nv,)], "aba": [(nv,)], "rnea_parameters": [(nv,)], "aba_parameters": [(nv,)], "aba_locked": [(nv,), (nv,)],
            "rnea_bodies": [(nv,), (nj, 6), (nj, 6)], "aba_bodies": [(nv,), (nj, 6), (nj, 6)], "rnea_joint_wrenches": [(nv,), (nj, 6)],
            "aba_joint_wrenches": [(nv,), (nj, 6)], "rnea_crba": [(nv,), (nv, nv)], "integrate": [(nq,), (nv,), (nv,)],
            "aba_integrate": [(nv,), (nq,), (nv,)], "rnea_aba": [(nv,), (nv,)], "rnea_derivatives": [(nv,), (nv, nv), (nv, nv)],
            "aba_derivatives": [(nv,), (nv, nv), (nv, nv), (nv, nv)]}[name]


def bind(torch, hm, name, B, state, soa=False, pi=None):
    from mecano_amd import _lib
    ins = [state[k].clone() for k in STATE[name]] + ([pi.clone()] if pi is not None else [])
    if name in ("rnea", "aba", "aba_integrate", "rnea_bodies", "aba_bodies"):
        fn, args, keep, outs = prepare(torch, hm, name, B, ins, soa)
        return fn, list(args), keep[0], outs, keep
    dt = ins[0].dtype
    sfx = "f64" if dt == torch.float64 else "f32"
    x = [t.t().contiguous() if soa else t for t in ins]
    p = [t.data_ptr() for t in x]
    g, _ = hm._root(G)
    opts = hm._options(_lib.LAYOUT_SOA if soa else _lib.LAYOUT_AOS, stream=torch.cuda.current_stream().cuda_stream)
    if name == "integrate":
        args = [ctypes.c_double(DT), *p, ctypes.byref(opts)]
    else:
        args = [*p, g, None, ctypes.byref(opts)]
    outs = [_out(torch, B, s, dt, soa) for s in out_shapes(hm, name)]
    return getattr(_lib.load(), f"mh_{name}_{sfx}"), [hm._h, B, *args, *[o[2] for o in outs]], x, [o[:2] for o in outs], (x, g, opts)


def run(torch, fn, args):
    from mecano_amd import _lib
    _lib.check(fn(*args))
    torch.cuda.synchronize()


def as_rows(x, soa):
    return x.t() if soa else x


def check_alias(torch, hm, name, B, state, aliases, soa=False, pi=None, label="", written=True):
    """aliases: {output index: input index}.  The criterion of the module docstring."""
    fn, args, x0, outs0, _k0 = bind(torch, hm, name, B, state, soa, pi)
    before = [t.clone() for t in x0]
    run(torch, fn, args)
    for k, (rows, guard) in enumerate(outs0):
        assert torch.isnan(guard).all(), f"{label}: out-of-place call wrote past output {k}"
        assert not written or not torch.isnan(rows).any(), f"{label}: out-of-place call left rows of output {k} unwritten"
    for k, (t, b) in enumerate(zip(x0, before)):
        assert torch.equal(t, b), f"{label}: out-of-place call changed input {k}"
    fn, args, x1, outs1, _k1 = bind(torch, hm, name, B, state, soa, pi)
    n_out = len(outs1)
    for o, i in aliases.items():
        args[len(args) - n_out + o] = x1[i].data_ptr()
    run(torch, fn, args)
    for o in range(n_out):
        got = as_rows(x1[aliases[o]], soa) if o in aliases else outs1[o][0]
        if not torch.equal(got, outs0[o][0]):
            fn2, args2, _x2, outs2, _k2 = bind(torch, hm, name, B, state, soa, pi)  # is the plan reproducible out of place at all?
            run(torch, fn2, args2)
            again = all(torch.equal(a[0], b[0]) for a, b in zip(outs0, outs2))
            bad = (got != outs0[o][0]).reshape(B, -1).any(dim=1).nonzero().flatten()[:8].tolist()
            raise AssertionError(f"{label}: output {o} aliased to input {aliases.get(o)} differs from the out-of-place result in rows {bad} "
                                 f"(two out-of-place runs agree: {again})")
        if o not in aliases:
            assert torch.isnan(outs1[o][1]).all(), f"{label}: aliased call wrote past output {o}"
    for i, (t, b) in enumerate(zip(x1, before)):
        if i not in aliases.values():
            assert torch.equal(t, b), f"{label}: aliased call changed input {i}"


SIZES = ((1, 357), (3, 129), (None, 1), (None, 64))  # (MH_FAKE_CU_COUNT, B)


def sweep_sizes(torch, name_robot, dt, env, calls, sizes=SIZES, soa=False):
    """calls: [(entry point, {output: input}), ...] on one model per (switch set, fake CU count)"""
    rb = case(name_robot)
    for fake, B in sizes:
        e = dict(env, **({"MH_FAKE_CU_COUNT": fake} if fake else {}))
        hm = model(name_robot, **e)
        state = rb.device(torch, B, dt)
        for name, aliases in calls:
            check_alias(torch, hm, name, B, state, aliases, soa, label=f"{name_robot} {e} {name} {'soa' if soa else 'aos'} B={B} {aliases}")


ABA_PLANS = {
    "bias_split": {"MH_ZV": 2},
    "fused": {"MH_ZV": 0, "MH_ZVF": 2},
    "two_launch": {"MH_ZV": 0, "MH_ZVF": 0, "MH_ZVB": 2},
    "tree_split": {"MH_ZV": 0, "MH_ZVF": 0, "MH_ZVB": 0},
    "tree_split_direct": {"MH_ZV": 0, "MH_ZVF": 0, "MH_ZVB": 0, "MH_SPEC_IO": 0},
    "whole_tree": {"MH_SPEC_SPLIT": 0},
    "whole_tree_st0": {"MH_SPEC_SPLIT": 0, "MH_SPEC_ST": 0},
    "whole_tree_st1": {"MH_SPEC_SPLIT": 0, "MH_SPEC_ST": 1},
    "run_time_split": {"MH_DISABLE_SPEC": 1, "MH_SPLIT_RT": 1},
    "sweep": {"MH_DISABLE_SPEC": 1, "MH_SPLIT_RT": 0},
    "depth_first": {"MH_DISABLE_SPEC": 1, "MH_SPLIT_RT": 0, "MH_DFS_ABA64": 1},
}
RNEA_PLANS = {
    "ahead": {"MH_RNEA_AHEAD": 2},
    "tree_split": {"MH_RNEA_AHEAD": 0},
    "whole_tree": {"MH_SPEC_SPLIT": 0},
    "run_time_split": {"MH_DISABLE_SPEC": 1, "MH_SPLIT_RT": 1},
    "depth_first": {"MH_DISABLE_SPEC": 1, "MH_SPLIT_RT": 0},
    "sweep": {"MH_DISABLE_SPEC": 1, "MH_SPLIT_RT": 0, "MH_DFS": 0},
}


@pytest.mark.parametrize("plan", list(ABA_PLANS))
def test_humanoid_forward_dynamics_in_place_on_every_plan(torch_cuda, plan):
    """mh_aba_f64 with qdd_out = tau and with qdd_out = qd (fp64, AoS), every plan of the table above."""
    torch = torch_cuda
    hm = model("humanoid", **ABA_PLANS[plan])
    assert hm.kernel_variant.startswith("generic" if "MH_DISABLE_SPEC" in ABA_PLANS[plan] else "topo:")
    sweep_sizes(torch, "humanoid", torch.float64, ABA_PLANS[plan], [("aba", {0: 2}), ("aba", {0: 1})])


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("plan", list(RNEA_PLANS))
def test_humanoid_inverse_dynamics_in_place_on_every_plan(torch_cuda, plan, soa):
    """mh_rnea_f64 with tau_out = qdd and with tau_out = qd (fp64), AoS and SoA."""
    torch = torch_cuda
    sweep_sizes(torch, "humanoid", torch.float64, RNEA_PLANS[plan], [("rnea", {0: 2}), ("rnea", {0: 1})], soa=soa)


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_tree128_in_place_on_the_run_time_kernels(torch_cuda, precision, soa):
    """The 128-body tree: depth-first walks (LDS row windows of the AoS inverse dynamics), transposed scratch copies, the sweep kernels and
    the run-time tree split, both algorithms, the output as the third input and as qd."""
    torch = torch_cuda
    dt = torch.float32 if precision == "f32" else torch.float64
    calls = [(n, {0: i}) for n in ("rnea", "aba") for i in (2, 1)]
    sweep_sizes(torch, "tree128", dt, {}, calls, sizes=((1, 357), (None, 64), (None, 1)), soa=soa)
    sweep_sizes(torch, "tree128", dt, {"MH_GENERIC_TRANSPOSE": 1}, calls, sizes=((3, 64 * 7 + 5),), soa=soa)
    sweep_sizes(torch, "tree128", dt, {"MH_DFS": 0}, calls, sizes=((1, 357),), soa=soa)


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("spec", [True, False])
def test_arm7_output_as_q(torch_cuda, spec, precision, soa):
    """nq == nv, every joint revolute with its row of q being its row of qd: the output may be q itself (and qd, and the third input)."""
    torch = torch_cuda
    dt = torch.float32 if precision == "f32" else torch.float64
    env = {} if spec else {"MH_DISABLE_SPEC": 1}
    assert model("arm7", **env).kernel_variant.startswith("topo:" if spec else "generic")
    calls = [(n, {0: i}) for n in ("rnea", "aba") for i in (0, 1, 2)]
    sweep_sizes(torch, "arm7", dt, env, calls, soa=soa)
    if spec and precision == "f64" and not soa:  # the whole-tree forward dynamics with its hand-over in LDS and in the global workspace
        for st in (0, 1):
            sweep_sizes(torch, "arm7", dt, {"MH_SPEC_ST": st}, calls, sizes=((1, 357), (None, 64)))


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_revolute_tree_output_as_q(torch_cuda, precision, soa):
    """A branching revolute tree (nq == nv) on the run-time kernels: the tree split over four waves, where every wave reads the trunk's
    rows of q (MH_SPLIT_RT=1 at every size), the depth-first walks and the sweep kernels; the output as q, and as the other two."""
    torch = torch_cuda
    dt = torch.float32 if precision == "f32" else torch.float64
    assert "run-time tree split" in model("rev14", MH_SPLIT_RT=1).kernel_variant  # (the tree has a usable split plan)
    calls = [(n, {0: i}) for n in ("rnea", "aba") for i in (0, 1, 2)]
    sweep_sizes(torch, "rev14", dt, {"MH_SPLIT_RT": 1}, calls, soa=soa)
    sweep_sizes(torch, "rev14", dt, {"MH_SPLIT_RT": 0}, calls, sizes=((1, 357), (None, 64)), soa=soa)
    sweep_sizes(torch, "rev14", dt, {"MH_SPLIT_RT": 0, "MH_DFS": 0}, calls, sizes=((1, 357),), soa=soa)


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_permuted_index_maps_in_place(torch_cuda, precision, soa):
    """Non-identity index maps (no identity-map plan, no dense staging): the output as the third input and as qd."""
    torch = torch_cuda
    dt = torch.float32 if precision == "f32" else torch.float64
    calls = [(n, {0: i}) for n in ("rnea", "aba") for i in (2, 1)]
    sweep_sizes(torch, "perm12", dt, {}, calls, soa=soa)
    sweep_sizes(torch, "perm12", dt, {"MH_DFS": 0, "MH_SPLIT_RT": 0}, calls, sizes=((1, 357),), soa=soa)


def parameters_of(torch, rb, B, dt):
    import inertial_parameters_check as ipc
    pool = ipc.physical_parameter_sets(rb.d, np.random.default_rng(61), 7).reshape(7, -1)
    return torch.tensor(pool, device="cuda", dtype=dt)[torch.arange(B, device="cuda") % 7].contiguous()


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name_robot", ["humanoid", "mixed"])
def test_parameter_calls_in_place(torch_cuda, name_robot, precision, soa):
    """mh_*_parameters_*: the output as the third input and as qd."""
    torch = torch_cuda
    dt = torch.float32 if precision == "f32" else torch.float64
    rb = case(name_robot)
    for fake, B in ((1, 357), (None, 64)):
        hm = model(name_robot, **({"MH_FAKE_CU_COUNT": fake} if fake else {}))
        state, pi = rb.device(torch, B, dt), parameters_of(torch, rb, B, dt)
        for name in ("rnea_parameters", "aba_parameters"):
            for i in (2, 1):
                check_alias(torch, hm, name, B, state, {0: i}, soa, pi, label=f"{name_robot} {name} {precision} soa={soa} B={B} out=in{i}")


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("locked", ["none", "every_third", "all"])
@pytest.mark.parametrize("name_robot", ["humanoid", "mixed"])
def test_locked_forward_dynamics_in_place(torch_cuda, name_robot, locked, precision, soa):
    """mh_aba_locked_*: qdd_out = qdd_in and tau_out = tau at once."""
    torch = torch_cuda
    dt = torch.float32 if precision == "f32" else torch.float64
    rb = case(name_robot)
    n = rb.d.n_joints
    from mecano_amd.engine import HipModel
    hm = HipModel(rb.d)  # a model of its own: the source modes belong to it
    modes = {"none": np.zeros(n), "every_third": (np.arange(n) % 3 == 0), "all": np.ones(n)}[locked].astype(np.int32)
    hm.set_joint_source_modes(modes)
    for B in (357, 64, 1):
        check_alias(torch, hm, "aba_locked", B, rb.device(torch, B, dt), {0: 3, 1: 2}, soa, label=f"{name_robot} locked {locked} {precision} soa={soa} B={B}")


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("name_robot", ["humanoid", "mixed"])
def test_per_body_and_per_joint_calls_in_place(torch_cuda, name_robot, soa):
    """mh_*_bodies_* (both precisions) and mh_*_joint_wrenches_f64: tau_out / qdd_out as the third input and as qd, the per-body outputs
    apart.  mh_aba_joint_wrenches_f64 takes qdd_out = tau only: its second launch reads q and qd again."""
    torch = torch_cuda
    rb = case(name_robot)
    for env in ({}, {"MH_DISABLE_SPEC": 1, "MH_FAKE_CU_COUNT": 1}):
        hm = model(name_robot, **env)
        for dt in (torch.float64, torch.float32):
            for B in (357, 64):
                state = rb.device(torch, B, dt)
                names = ("rnea_bodies", "aba_bodies") + (("rnea_joint_wrenches", "aba_joint_wrenches") if dt == torch.float64 else ())
                for name in names:
                    for i in (2,) if name == "aba_joint_wrenches" else (2, 1):
                        check_alias(torch, hm, name, B, state, {0: i}, soa, label=f"{name_robot} {env} {name} {dt} soa={soa} B={B} out=in{i}")


@pytest.mark.parametrize("spec", [True, False])
@pytest.mark.parametrize("name_robot", ["humanoid", "mixed"])
def test_rnea_crba_with_tau_out_as_qdd(torch_cuda, name_robot, spec):
    """mh_rnea_crba_f64: the mass matrix reads q only, so tau_out may be qdd (or qd) -- one launch with a code object, two without."""
    torch = torch_cuda
    rb = case(name_robot)
    for fake, B in ((1, 357), (None, 64), (None, 1)):
        env = dict({} if spec else {"MH_DISABLE_SPEC": 1}, **({"MH_FAKE_CU_COUNT": fake} if fake else {}))
        hm = model(name_robot, **env)
        for i in (2, 1):
            check_alias(torch, hm, "rnea_crba", B, rb.device(torch, B, torch.float64), {0: i}, label=f"{name_robot} {env} rnea_crba B={B} tau_out=in{i}")


@pytest.mark.parametrize("soa", [False, True])
@pytest.mark.parametrize("name_robot", ["humanoid", "mixed"])
def test_integrate_f32_in_place(torch_cuda, name_robot, soa):
    """mh_integrate_f32 (and _f64) with every output as its own input.  Entries no joint owns are not written."""
    torch = torch_cuda
    rb = case(name_robot)
    hm = model(name_robot)
    for dt in (torch.float32, torch.float64):
        for B in (357, 64, 1):
            check_alias(torch, hm, "integrate", B, rb.device(torch, B, dt), {0: 0, 1: 1, 2: 2}, soa, label=f"{name_robot} integrate {dt} soa={soa} B={B}")


@pytest.mark.parametrize("env", [{}, {"MH_ZV_STEP": 0}, {"MH_SPEC_SPLIT": 0}, {"MH_DISABLE_SPEC": 1}], ids=str)
def test_simulation_step_in_place(torch_cuda, env):
    """mh_aba_integrate_f64 with q_next = q and qd_next = qd: the step riding in the bias-split / fused launches (default), in the tree-split
    kernel (MH_ZV_STEP=0: use_zv_step keeps the step out of the zv plans), and as two launches (MH_SPEC_SPLIT=0, no code object)."""
    torch = torch_cuda
    sweep_sizes(torch, "humanoid", torch.float64, env, [("aba_integrate", {1: 0, 2: 1})])


# ======================================================================== refusals
def arena_bind(torch, hm, name, B, state, dt, pi=None, f_ext=False):
    """Every input and output of one call inside ONE poisoned buffer with room behind it for the largest output: whatever pointer a case
    passes, a call that was wrongly let through would still write inside the buffer.  (arena, input views, output views, arguments,
    positions of the inputs / outputs among the arguments, keep)"""
    from mecano_amd import _lib
    ins = [state[k] for k in STATE[name]] + ([pi] if pi is not None else [])
    if f_ext:
        ins.append(torch.rand((B, hm.n_joints * 6), device="cuda", dtype=torch.float64).to(dt))
    shapes = out_shapes(hm, name)
    sizes = [t.numel() for t in ins] + [B * int(np.prod(s)) for s in shapes]
    arena = torch.full((sum(sizes) + max(sizes),), float("nan"), device="cuda", dtype=dt)
    views, ofs = [], 0
    for n in sizes:
        views.append(arena[ofs:ofs + n])
        ofs += n
    x = [v.view(t.shape) for v, t in zip(views, ins)]
    for v, t in zip(x, ins):
        v.copy_(t)
    outs = [v.view(B, *s) for v, s in zip(views[len(ins):], shapes)]
    g, _ = hm._root(G)
    opts = hm._options(_lib.LAYOUT_AOS, stream=torch.cuda.current_stream().cuda_stream)
    n_state = len(STATE[name]) + (1 if pi is not None else 0)
    p = [t.data_ptr() for t in x]
    fp = p[-1] if f_ext else None
    head = [ctypes.c_double(DT)] if name in ("integrate", "aba_integrate") else []
    tail = [ctypes.byref(opts)] if name == "integrate" else [g, fp, ctypes.byref(opts)]
    args = [hm._h, B, *head, *p[:n_state], *tail, *[o.data_ptr() for o in outs]]
    sfx = "f64" if dt == torch.float64 else "f32"
    fn = getattr(_lib.load(), f"mh_{name}_{sfx}")
    return arena, x, outs, fn, args, len(args) - len(outs), (g, opts, ins)


# (entry point, precisions, robot, [(what, {output index: (input | output, index, rows past its start)}), ...]); input indices follow the
# call's argument order, "f" is f_ext, and for the parameter calls the last state input is pi
ONE = [("partial overlap with qd", {0: ("in", 1, 1)}), ("partial overlap with the third input", {0: ("in", 2, 1)}),
       ("partial overlap with q", {0: ("in", 0, 1)}), ("q of another shape (nq != nv)", {0: ("in", 0, 0)}), ("f_ext", {0: ("f", 0, 0)})]
BODIES = [("partial overlap with qdd / tau", {0: ("in", 2, 1)}), ("body_acc_out over qd", {1: ("in", 1, 0)}), ("body_twist_out over q", {2: ("in", 0, 0)}),
          ("body_twist_out over body_acc_out", {2: ("out", 1, 0)}), ("body_acc_out over the joint output", {1: ("out", 0, 0)}), ("body_acc_out over f_ext", {1: ("f", 0, 0)})]
WRENCHES = [("partial overlap with qd", {0: ("in", 1, 1)}), ("joint_wrench_out over the third input", {1: ("in", 2, 0)}), ("joint_wrench_out over q", {1: ("in", 0, 0)}),
            ("joint_wrench_out over the joint output", {1: ("out", 0, 0)})]


def every_pair(outs, ins, f_ext):
    """every (output, input) and (output, output) pair of a call whose outputs may be none of its inputs, each output at the start of the
    other argument"""
    pairs = [(f"{o} over {i}", {a: ("in", b, 0)}) for a, o in enumerate(outs) for b, i in enumerate(ins)]
    pairs += [(f"{o} over f_ext", {a: ("f", 0, 0)}) for a, o in enumerate(outs) if f_ext]
    return pairs + [(f"{o} over {p}", {a: ("out", b, 0)}) for a, o in enumerate(outs) for b, p in enumerate(outs) if b > a]


PAIR = every_pair(("tau_out", "qdd_out"), ("q", "qd", "qdd", "tau"), False) + [("partial overlap of qdd_out with tau", {1: ("in", 3, 1)})]
RNEA_DERIVATIVES = every_pair(("tau_out", "dtau_dq_out", "dtau_dqd_out"), ("q", "qd", "qdd"), True) \
    + [("partial overlap of dtau_dq_out with dtau_dqd_out", {1: ("out", 2, 1)})]
ABA_DERIVATIVES = every_pair(("qdd_out", "dqdd_dq_out", "dqdd_dqd_out", "Hinv_out"), ("q", "qd", "tau"), True) \
    + [("partial overlap of Hinv_out with qd", {3: ("in", 1, 1)})]
# (..., batch size) where it is not 70
REFUSALS = [
    ("rnea_aba", ("f64", "f32"), "humanoid", PAIR, 5), ("rnea_aba", ("f64", "f32"), "arm7", PAIR, 5),
    ("rnea_derivatives", ("f64", "f32"), "humanoid", RNEA_DERIVATIVES, 5), ("rnea_derivatives", ("f64", "f32"), "arm7", RNEA_DERIVATIVES, 5),
    ("aba_derivatives", ("f64", "f32"), "humanoid", ABA_DERIVATIVES, 5), ("aba_derivatives", ("f64", "f32"), "arm7", ABA_DERIVATIVES, 5),
    ("rnea", ("f64", "f32"), "humanoid", ONE), ("aba", ("f64", "f32"), "humanoid", ONE),
    ("rnea", ("f64", "f32"), "perm12", [("q where prismatic coordinates are read again", {0: ("in", 0, 0)})]),
    ("aba", ("f64", "f32"), "perm12", [("q where prismatic coordinates are read again", {0: ("in", 0, 0)})]),
    ("rnea_parameters", ("f64", "f32"), "humanoid", ONE[:3] + [("pi", {0: ("in", 3, 0)}), ("f_ext", {0: ("f", 0, 0)})]),
    ("aba_parameters", ("f64", "f32"), "mixed", ONE[:3] + [("pi", {0: ("in", 3, 0)}), ("f_ext", {0: ("f", 0, 0)})]),
    ("rnea_bodies", ("f64", "f32"), "humanoid", BODIES), ("aba_bodies", ("f64", "f32"), "mixed", BODIES),
    ("rnea_joint_wrenches", ("f64",), "humanoid", WRENCHES),
    ("aba_joint_wrenches", ("f64",), "humanoid", WRENCHES + [("qdd_out = qd, which the second launch reads", {0: ("in", 1, 0)})]),
    ("aba_joint_wrenches", ("f64",), "arm7", [("qdd_out = q, which the second launch reads", {0: ("in", 0, 0)}), ("qdd_out = qd", {0: ("in", 1, 0)})]),
    ("aba_locked", ("f64", "f32"), "humanoid", [("qdd_out = tau", {0: ("in", 2, 0)}), ("qdd_out = qd", {0: ("in", 1, 0)}), ("tau_out = qdd_in", {1: ("in", 3, 0)}),
                                                 ("tau_out = qd", {1: ("in", 1, 0)}), ("qdd_out = tau_out", {0: ("out", 1, 0)}),
                                                 ("partial overlap of qdd_out with qdd_in", {0: ("in", 3, 1)}), ("partial overlap of tau_out with tau", {1: ("in", 2, 1)}),
                                                 ("qdd_out over f_ext", {0: ("f", 0, 0)})]),
    ("aba_locked_some", ("f64", "f32"), "humanoid", [("qdd_out = tau", {0: ("in", 2, 0)}), ("tau_out = qdd_in", {1: ("in", 3, 0)})]),
    ("rnea_crba", ("f64",), "arm7", [("tau_out = q", {0: ("in", 0, 0)}), ("H_out over q", {1: ("in", 0, 0)}), ("H_out over qd", {1: ("in", 1, 0)}),
                                     ("H_out over tau_out", {1: ("out", 0, 0)}), ("partial overlap of tau_out with qdd", {0: ("in", 2, 1)}),
                                     ("H_out over f_ext", {1: ("f", 0, 0)})]),
    ("integrate", ("f64", "f32"), "humanoid", [("q_out over qd", {0: ("in", 1, 0)}), ("qd_out = qdd", {1: ("in", 2, 0)}), ("qdd_out = qd", {2: ("in", 1, 0)}),
                                                ("partial overlap of q_out with q", {0: ("in", 0, 1)}), ("qd_out = qdd_out", {1: ("out", 2, 0)})]),
    ("aba_integrate", ("f64",), "humanoid", [("qdd_out = tau", {0: ("in", 2, 0)}), ("qdd_out = qd", {0: ("in", 1, 0)}), ("qdd_out = qd_next", {0: ("out", 2, 0)}),
                                              ("partial overlap of q_next with q", {1: ("in", 0, 1)}), ("qd_next = tau", {2: ("in", 2, 0)}),
                                              ("q_next over f_ext", {1: ("f", 0, 0)})]),
]


@pytest.mark.parametrize("entry", REFUSALS, ids=lambda e: f"{e[0]}-{e[2]}")
def test_forbidden_overlaps_are_refused(torch_cuda, entry):
    """Every forbidden overlap of the header: MH_ERR_INVALID_ARGUMENT, "overlap" in mh_last_error, nothing written (the poisoned outputs and
    everything behind them still NaN after a synchronise, the inputs as they were), and the next valid call on the model is right."""
    torch = torch_cuda
    from mecano_amd import _lib
    from mecano_amd.engine import HipModel
    name, precisions, name_robot, cases = entry[:4]
    rb = case(name_robot)
    some_locked = name == "aba_locked_some"
    name = "aba_locked" if some_locked else name
    if some_locked:
        hm = HipModel(rb.d)
        hm.set_joint_source_modes((np.arange(rb.d.n_joints) % 3 == 0).astype(np.int32))
    else:
        hm = model(name_robot)
    B = entry[4] if len(entry) > 4 else 70
    lib = _lib.load()
    for sfx in precisions:
        dt = torch.float64 if sfx == "f64" else torch.float32
        state = rb.device(torch, B, dt)
        pi = parameters_of(torch, rb, B, dt) if "parameters" in name else None
        fn0, args0, _x0, outs0, _k0 = bind(torch, hm, name, B, state, False, pi)  # what the valid call gives (no external wrenches)
        run(torch, fn0, args0)
        for what, moves in cases:
            f_ext = any(m[0] == "f" for m in moves.values())
            arena, x, outs, fn, args, first_out, keep = arena_bind(torch, hm, name, B, state, dt, pi, f_ext)
            snapshot = arena.clone()
            for o, (kind, i, rows_past) in moves.items():
                base = x[-1] if kind == "f" else (x[i] if kind == "in" else outs[i])
                args[first_out + o] = base.data_ptr() + rows_past * base[0].numel() * base.element_size()
            status = fn(*args)
            message = lib.mh_last_error().decode()
            torch.cuda.synchronize()
            assert status == INVALID, f"mh_{name}_{sfx}: {what}: status {status} ({message})"
            assert "overlap" in message, f"mh_{name}_{sfx}: {what}: {message}"
            same = (arena == snapshot) | (torch.isnan(arena) & torch.isnan(snapshot))
            assert bool(same.all()), f"mh_{name}_{sfx}: {what}: the refused call wrote something"
            assert all(bool(torch.isnan(o).all()) for o in outs), f"mh_{name}_{sfx}: {what}: outputs touched"
            if f_ext:
                continue  # (the valid call below is compared with a call without external wrenches)
            arena, x, outs, fn, args, first_out, keep = arena_bind(torch, hm, name, B, state, dt, pi)
            run(torch, fn, args)
            for k, (o, (ref, _g)) in enumerate(zip(outs, outs0)):
                assert torch.equal(o, ref), f"mh_{name}_{sfx}: the valid call after '{what}': output {k} differs"
