"""Every row group of device-filling batches: the persistent and grid-stride loops of the HIP kernels against the fp64 CPU oracle.

At device-filling batch sizes a workgroup takes group g of 64 configurations, then g + grid, g + 2 grid, ...  The inputs here are distinct
on every row (tests/helpers.py: DistinctRows -- a row read from the wrong iteration holds another state), the outputs are poisoned with NaN
and have a guard row behind the last one, and the rows checked against the oracle touch every group of 64 (helpers.group_cover).

Tier A: the real CU count, batch sizes one row below, at and above each switch point of the dispatcher and k grid 64 + 37 (a ragged last
iteration), each case forcing the plan it means to reach where a switch exists.  Tier B: MH_FAKE_CU_COUNT = 1, 3, 5 (grids shrunk, never
grown) at a few hundred to three thousand configurations, so that every loop runs several iterations over odd grids, every row checked.
The reserve-then-capture test at the end holds mh_reserve to its header's promise for the depth-first plans."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from helpers import (DistinctRows, check_cover, close_aba, f32_aba_backward_tol, f32_forward_tol, group_cover, poisoned,
                     record_parity)

pytestmark = pytest.mark.gpu

G = (0.3, -0.2, -9.81)
DT = 1.0e-3
KEYS = ("MH_DISABLE_SPEC", "MH_ZV", "MH_ZVF", "MH_ZVB", "MH_ZVF_PAIR", "MH_RNEA_AHEAD", "MH_SPEC_SPLIT", "MH_CRBA_LPG", "MH_DFS_PAIR",
        "MH_SPLIT_RT", "MH_FAKE_CU_COUNT")


@pytest.fixture(scope="module")
def torch_cuda(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def cu(torch_cuda):
    return int(torch_cuda.cuda.get_device_properties(0).multi_processor_count)


@contextlib.contextmanager
def switches(**env):
    """The MH_* switches are read at model creation: set them, create the model inside, restore them after."""
    saved = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Robot:
    def __init__(self, name):
        from mecano_amd import random_tools as rt
        from oracle.cpu_oracle import OracleModel
        if name == "humanoid":
            self.sys = rt.nextHumanoid(np.random.default_rng(43))
            self.rows = DistinctRows(self.sys, 1024, 2342)
        else:
            from mecano_amd.multibody import MultiBodySystem
            joints = rt.nextJointTree(np.random.default_rng(128), 128, ("revolute", "prismatic", "sixdof"))
            self.sys = MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor())
            self.rows = DistinctRows(self.sys, 2048, 2342)
        self.d = self.sys.toModelDesc()
        self.om = OracleModel(self.d)
        self.n = self.d.n_joints
        self._memo = {}

    def per_row(self, key, idx, compute):
        """compute(rows) -> a list of [len(rows), ...] arrays for rows idx; each row is computed once per key (row r holds the same state at
        every batch size)"""
        memo = self._memo.setdefault(key, {})
        idx = np.asarray(idx, dtype=np.int64).tolist()
        todo = [r for r in idx if r not in memo]
        if todo:
            outs = compute(np.array(todo, dtype=np.int64))
            for j, r in enumerate(todo):
                memo[r] = [o[j] for o in outs]
        return [np.stack([memo[r][k] for r in idx]) for k in range(len(memo[idx[0]]))]

    def model(self, **env):
        from mecano_amd.engine import HipModel
        with switches(**env):
            return HipModel(self.d)


_ROBOTS = {}


def robot(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = Robot(name)
    return _ROBOTS[name]


def below_at_above(first):
    """one row below the first batch size of a plan, that size and one row above"""
    return [first - 1, first, first + 1]


# ---- the calls, on poisoned outputs with a guard row (SoA: [n][B] matrices, the guard is n more entries behind them)
def _out(torch, B, shape, dt, soa):
    """(rows view [B, ...], guard, device pointer the call writes to)"""
    if not soa:
        rows, guard = poisoned(torch, B, shape, dt)
        return rows, guard, rows.data_ptr()
    mat, guard = poisoned(torch, int(np.prod(shape)), (B,), dt)
    return mat.t(), guard, mat.data_ptr()


def prepare(torch, hm, name, B, ins, soa=False):
    """Entry point `name` bound to device inputs ins (AoS [B, n]; transposed copies for SoA) and poisoned outputs on the current stream:
    (function, arguments, what the arguments point to (inputs as passed, gravity, options), [(rows, guard), ...])."""
    from mecano_amd import _lib
    lib = _lib.load()
    dt = ins[0].dtype
    sfx = "f64" if dt == torch.float64 else "f32"
    x = [t.t().contiguous() if soa else t for t in ins]
    p = [t.data_ptr() for t in x]
    g, _ = hm._root(G)
    opts = hm._options(_lib.LAYOUT_SOA if soa else _lib.LAYOUT_AOS, stream=torch.cuda.current_stream().cuda_stream)
    nv, nj = hm.nv, hm.n_joints
    if name in ("rnea", "aba"):
        shapes, args = [(nv,)], (p[0], p[1], p[2], g, None, ctypes.byref(opts))
    elif name == "rnea_aba":
        shapes, args = [(nv,), (nv,)], (p[0], p[1], p[2], p[3], g, None, ctypes.byref(opts))
    elif name == "crba":
        shapes, args = [(nv, nv)], (p[0], ctypes.byref(opts))
    elif name == "crba_coriolis":
        shapes, args = [(nv, nv), (nv, nv)], (p[0], p[1], ctypes.byref(opts))
    elif name == "centroidal":
        shapes, args = [(6, nv), (6,), (3,)], (p[0], p[1], None, _lib.CENTROIDAL_FRAME_FIXED, ctypes.byref(opts))
    elif name == "aba_integrate":
        shapes, args = [(nv,), (hm.nq,), (nv,)], (ctypes.c_double(DT), p[0], p[1], p[2], g, None, ctypes.byref(opts))
    elif name in ("rnea_bodies", "aba_bodies"):
        shapes, args = [(nv,), (nj, 6), (nj, 6)], (p[0], p[1], p[2], g, None, ctypes.byref(opts))
    else:
        raise ValueError(name)
    outs = [_out(torch, B, s, dt, soa) for s in shapes]
    keep = (x, g, opts)
    return getattr(lib, f"mh_{name}_{sfx}"), (hm._h, B, *args, *[o[2] for o in outs]), keep, [o[:2] for o in outs]


def invoke(torch, hm, name, B, ins, soa=False):
    """Runs entry point `name` on device inputs into poisoned outputs: [(rows, guard), ...]."""
    from mecano_amd import _lib
    fn, args, _keep, outs = prepare(torch, hm, name, B, ins, soa)
    _lib.check(fn(*args))
    torch.cuda.synchronize()
    return outs


def oracle(rb, name, idx, dtype=np.float64):
    """the oracle's outputs of entry point `name` on rows idx (inputs rounded to `dtype`), each row computed once"""
    return rb.per_row((name, np.dtype(dtype).name), idx, lambda rows: _oracle(rb, name, rows, dtype))


def _oracle(rb, name, idx, dtype):
    q, qd, qdd, tau = rb.rows.rows(idx, dtype)
    om = rb.om
    if name == "rnea":
        return [om.rnea(q, qd, qdd, G)]
    if name == "bias":
        return [om.rnea(q, qd, np.zeros_like(qdd), G)]
    if name == "aba":
        return [om.aba(q, qd, tau, G)]
    if name == "rnea_aba":
        return [om.rnea(q, qd, qdd, G), om.aba(q, qd, tau, G)]
    if name == "crba":
        return [om.crba(q)]
    if name == "crba_coriolis":
        return list(om.crba_coriolis(q, qd))
    if name == "centroidal":
        return list(om.centroidal(q, qd))
    if name == "aba_integrate":
        a = om.aba(q, qd, tau, G)
        qn, vn, _ = om.integrate(DT, q, qd, a)
        return [a, qn, vn]
    if name == "rnea_bodies":
        return list(om.rnea_bodies(q, qd, qdd, G))
    if name == "aba_bodies":
        return list(om.aba_bodies(q, qd, tau, G))
    raise ValueError(name)


# inputs of each entry point among (q, qd, qdd, tau)
INPUTS = {"rnea": (0, 1, 2), "aba": (0, 1, 3), "rnea_aba": (0, 1, 2, 3), "crba": (0,), "crba_coriolis": (0, 1), "centroidal": (0, 1),
          "aba_integrate": (0, 1, 3), "rnea_bodies": (0, 1, 2), "aba_bodies": (0, 1, 3)}
# ABA's outputs are held to the absolute 1e-10 on the humanoid (BASELINE's north star, as the neighbouring tests do); its per-body
# accelerations to 1e-9 relative (test_per_body_outputs_from_the_tree_split_kernels)
TOL64 = {"aba_bodies": (1e-10, 1e-9, 1e-10)}


def check_fp64(torch, rb, hm, name, B, label, grid=None, every=False, soa=False):
    """One call of `name` at batch B on distinct rows, checked on the group cover (every=True: every row) against the oracle in fp64."""
    ins = rb.rows.device(torch, B)
    outs = invoke(torch, hm, name, B, [ins[k] for k in INPUTS[name]], soa)
    idx = np.arange(B) if every else group_cover(B, grid)
    refs = oracle(rb, name, idx)
    tols = TOL64.get(name, (1e-10,) * len(refs))
    for k, ((rows, guard), ref) in enumerate(zip(outs, refs)):
        if rb.n > 64 and name in ("aba", "rnea_aba") and k == len(refs) - 1:  # the deep random tree: forward dynamics by cond(H) of each row
            check_cover(rows, guard, idx, ref, np.inf, label=f"{label} out{k} (rows written)", record=False)
            conds = rb.per_row("cond_inf(H)", idx, lambda r: [np.array([np.linalg.cond(H, np.inf) for H in rb.om.crba(rb.rows.rows(r)[0])])])[0]
            close_aba(rows[torch.as_tensor(idx, device="cuda")].cpu().numpy(), ref, None, rb.n, label=f"{label} out{k}", conds=conds)
            continue
        absolute = rb.n < 64 and name in ("aba", "rnea_aba", "aba_integrate") and k == (len(refs) - 1 if name == "rnea_aba" else 0)
        check_cover(rows, guard, idx, ref, tols[k], absolute=absolute, label=f"{label} out{k}")


def check_fp32(torch, rb, hm, name, B, label, grid=None, every=False, soa=False):
    """fp32 RNEA / ABA / the pair call of the 128-body tree: efforts by the derived forward bound, accelerations by their backward error."""
    ins = rb.rows.device(torch, B, torch.float32)
    outs = invoke(torch, hm, name, B, [ins[k] for k in INPUTS[name]], soa)
    idx = np.arange(B) if every else group_cover(B, grid)
    q, qd, qdd, tau = rb.rows.rows(idx, np.float32)
    om, n = rb.om, rb.n
    kinds = {"rnea": ["tau"], "aba": ["qdd"], "rnea_aba": ["tau", "qdd"]}[name]
    for (rows, guard), kind in zip(outs, kinds):
        if kind == "tau":
            check_cover(rows, guard, idx, oracle(rb, "rnea", idx, np.float32)[0], f32_forward_tol(n), label=f"{label} tau")
            continue
        check_cover(rows, guard, idx, np.zeros((len(idx), rb.d.nv)), np.inf, label=f"{label} qdd (rows written)", record=False)
        a32 = rows[torch.as_tensor(idx, device="cuda")].cpu().numpy().astype(np.float64)
        bias = oracle(rb, "bias", idx, np.float32)[0]
        scale = np.abs(tau).max() + np.abs(bias).max()
        berr = np.abs(om.rnea(q, qd, a32, G) - tau).max()
        record_parity(berr, f32_aba_backward_tol(n) * scale, f"{label} qdd backward error")
        assert berr <= f32_aba_backward_tol(n) * scale, (label, berr, scale)


# ======================================================================== Tier A: the real CU count
def test_humanoid_forward_dynamics_plans(torch_cuda, cu):
    """ABA on the humanoid's code object.  Fused one-launch forward dynamics (zvf: groups = min(ceil(B/64), 2 cu), from ceil(B/64) > cu);
    the two-launch form (zvb, MH_ZVF=0, from ceil(B/64) >= 2 cu); the one-job tree-split kernel (MH_ZVF=0 MH_ZVB=0, grid 2 cu); and the
    simulation step on top of the default plan."""
    torch = torch_cuda
    rb = robot("humanoid")
    hm = rb.model()
    assert hm.kernel_variant.startswith("topo:")
    loop = 2 * cu * 64
    for B in below_at_above(cu * 64 + 1) + [loop + 37, 2 * loop + 37]:
        check_fp64(torch, rb, hm, "aba", B, f"aba zvf {B}", grid=2 * cu)
    for B in (cu * 64 + 1, loop + 37):
        check_fp64(torch, rb, hm, "aba_integrate", B, f"step {B}", grid=2 * cu)
    zvb = rb.model(MH_ZV=0, MH_ZVF=0, MH_ZVB=2)
    for B in below_at_above((2 * cu - 1) * 64 + 1) + [2 * loop + 37]:
        check_fp64(torch, rb, zvb, "aba", B, f"aba zvb {B}", grid=2 * cu)
    one_job = rb.model(MH_ZV=0, MH_ZVF=0, MH_ZVB=0)
    check_fp64(torch, rb, one_job, "aba", 2 * loop + 37, f"aba tree-split {2 * loop + 37}", grid=2 * cu)


def test_humanoid_inverse_dynamics_and_pair_plans(torch_cuda, cu):
    """RNEA in the loop that requests rows ahead (from ceil(B/64) > 2 cu; MH_RNEA_AHEAD=2 forces it below, 0 keeps the tree-split loop), the
    pair call (one fused launch beyond ceil(B/64) > cu; MH_ZVF_PAIR=0 the two launches), the per-body variants and SoA."""
    torch = torch_cuda
    rb = robot("humanoid")
    hm = rb.model()
    loop = 2 * cu * 64
    for B in below_at_above(loop + 1) + [2 * loop + 37]:
        check_fp64(torch, rb, hm, "rnea", B, f"rnea {B}", grid=2 * cu)
    ahead = rb.model(MH_RNEA_AHEAD=2)
    check_fp64(torch, rb, ahead, "rnea", loop // 2 + 37, f"rnea ahead forced {loop // 2 + 37}", grid=2 * cu)
    no_ahead = rb.model(MH_RNEA_AHEAD=0)
    check_fp64(torch, rb, no_ahead, "rnea", 2 * loop + 37, f"rnea tree-split {2 * loop + 37}", grid=2 * cu)
    for B in below_at_above(cu * 64 + 1) + [loop + 37, 2 * loop + 37]:
        check_fp64(torch, rb, hm, "rnea_aba", B, f"pair {B}", grid=2 * cu)
    two = rb.model(MH_ZVF_PAIR=0)
    check_fp64(torch, rb, two, "rnea_aba", loop + 37, f"pair two launches {loop + 37}", grid=2 * cu)
    for name in ("rnea_bodies", "aba_bodies"):
        check_fp64(torch, rb, hm, name, 2 * loop + 37, f"{name} {2 * loop + 37}", grid=2 * cu)
    for name in ("rnea", "aba"):
        check_fp64(torch, rb, hm, name, 2 * loop + 37, f"{name} soa {2 * loop + 37}", grid=2 * cu, soa=True)


def test_humanoid_crba_coriolis_centroidal_loops(torch_cuda, cu):
    """Tree-split CRBA (ng = ceil(B / width) workgroups capped at 2 cu: the loop iterates beyond 32 cu configurations at width 64, the
    default there, and MH_CRBA_LPG=16 beyond 8 cu), the whole-wave packed CRBA (MH_SPEC_SPLIT=0); mass + Coriolis and centroidal momentum
    (grids capped at 4 cu waves: they iterate beyond 256 cu configurations)."""
    torch = torch_cuda
    rb = robot("humanoid")
    hm = rb.model()
    loop = 2 * cu * 64
    for B in (loop + 1, 2 * loop + 37):
        check_fp64(torch, rb, hm, "crba", B, f"crba {B}", grid=2 * cu)
    for env, B in (({"MH_CRBA_LPG": 64}, loop + 37), ({"MH_CRBA_LPG": 16}, loop // 4 + 37), ({"MH_SPEC_SPLIT": 0}, loop + 37)):
        check_fp64(torch, rb, rb.model(**env), "crba", B, f"crba {env} {B}", grid=2 * cu)
    for B in below_at_above(4 * cu * 64 + 1) + [2 * 4 * cu * 64 + 37]:
        check_fp64(torch, rb, hm, "crba_coriolis", B, f"crba_coriolis {B}", grid=4 * cu)
        check_fp64(torch, rb, hm, "centroidal", B, f"centroidal {B}", grid=4 * cu)


def test_humanoid_on_the_run_time_kernels(torch_cuda, cu):
    """MH_DISABLE_SPEC=1: the run-time tree split up to ceil(B/64) <= 2 cu (grid 2 cu), the generic kernels above; MH_SPLIT_RT=1 keeps the
    tree split at every size."""
    torch = torch_cuda
    rb = robot("humanoid")
    hm = rb.model(MH_DISABLE_SPEC=1)
    assert hm.kernel_variant.startswith("generic")
    loop = 2 * cu * 64
    for B in below_at_above(loop + 1) + [2 * loop + 37]:
        for name in ("rnea", "aba", "rnea_aba"):
            check_fp64(torch, rb, hm, name, B, f"run-time {name} {B}", grid=2 * cu)
    check_fp64(torch, rb, hm, "crba", loop + 37, f"run-time crba {loop + 37}", grid=2 * cu)
    split = rb.model(MH_DISABLE_SPEC=1, MH_SPLIT_RT=1)
    for name in ("rnea", "aba"):
        check_fp64(torch, rb, split, name, 2 * loop + 37, f"run-time split forced {name} {2 * loop + 37}", grid=2 * cu)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_tree128_depth_first_loops(torch_cuda, cu, precision):
    """The 128-body tree on the run-time kernels: the tree split up to ceil(B/64) <= 2 cu, the depth-first walks (grids cu per_cu) above,
    the transposed copies of AoS rows from 8 192 configurations; in fp32 also mh_rnea_aba_f32 (one fused walk for big batches,
    MH_DFS_PAIR=0: two launches on shared copies), AoS and SoA, up to 131 072."""
    torch = torch_cuda
    rb = robot("tree128")
    hm = rb.model()
    check = check_fp32 if precision == "f32" else check_fp64
    loop = 2 * cu * 64
    sizes = below_at_above(8192) + below_at_above(loop + 1) + [131072 + 37] if precision == "f32" else [8191, 8193, loop + 1, 131072 + 37]
    for B in sizes:
        for soa in (False, True):
            lay = "soa" if soa else "aos"
            for name in ("rnea", "aba") + (("rnea_aba",) if precision == "f32" else ()):
                if B < 8000 and soa:
                    continue
                check(torch, rb, hm, name, B, f"tree128 {precision} {name} {lay} {B}", grid=cu, soa=soa)
    if precision == "f32":
        two = rb.model(MH_DFS_PAIR=0)
        for soa in (False, True):
            check(torch, rb, two, "rnea_aba", 131072 + 37, f"tree128 f32 pair MH_DFS_PAIR=0 {'soa' if soa else 'aos'} 131109", grid=cu, soa=soa)


# ======================================================================== Tier B: shrunk grids, many iterations, every row
@pytest.mark.parametrize("fake", [1, 3, 5])
def test_humanoid_loops_on_shrunk_grids(torch_cuda, cu, fake):
    """MH_FAKE_CU_COUNT shrinks every grid: the humanoid's fused / two-launch forward dynamics, the ahead-requesting RNEA, the pair call,
    CRBA, mass + Coriolis, centroidal, the step and the per-body variants loop 3 - 20 times over odd grids with ragged tails; the run-time
    kernels likewise.  Every row against the oracle."""
    assert fake <= cu
    torch = torch_cuda
    rb = robot("humanoid")
    sizes = {1: (300, 1000 + 37), 3: (1200 + 5, 2000 + 37), 5: (2900 + 37,)}[fake]
    plans = [({}, ("rnea", "aba", "rnea_aba", "crba", "crba_coriolis", "centroidal", "aba_integrate", "rnea_bodies", "aba_bodies")),
             ({"MH_ZV": 0, "MH_ZVF": 0, "MH_ZVB": 2}, ("aba",)), ({"MH_RNEA_AHEAD": 2}, ("rnea",)), ({"MH_CRBA_LPG": 16}, ("crba",)),
             ({"MH_DISABLE_SPEC": 1}, ("rnea", "aba", "rnea_aba", "crba"))]
    for env, names in plans:
        hm = rb.model(MH_FAKE_CU_COUNT=fake, **env)
        for B in sizes:
            for name in names:
                check_fp64(torch, rb, hm, name, B, f"fake cu {fake} {env} {name} {B}", every=True)


@pytest.mark.parametrize("fake", [1, 3, 5])
def test_tree128_loops_on_shrunk_grids(torch_cuda, cu, fake):
    """The 128-body tree's depth-first walks and tree split on grids of 1 - 5 CUs (fp32 and fp64, AoS and SoA), every row; the fp32 fused pair
    walk at 8 229 configurations (its smallest batches) on group cover."""
    assert fake <= cu
    torch = torch_cuda
    rb = robot("tree128")
    B = {1: 700 + 37, 3: 1600 + 37, 5: 2600 + 37}[fake]
    hm = rb.model(MH_FAKE_CU_COUNT=fake)
    for soa in (False, True):
        lay = "soa" if soa else "aos"
        for name in ("rnea", "aba"):
            check_fp32(torch, rb, hm, name, B, f"fake cu {fake} tree128 f32 {name} {lay} {B}", every=True, soa=soa)
            check_fp64(torch, rb, hm, name, B, f"fake cu {fake} tree128 f64 {name} {lay} {B}", every=True, soa=soa)
        check_fp32(torch, rb, hm, "rnea_aba", 8192 + 37, f"fake cu {fake} tree128 f32 pair {lay} 8229", grid=fake * 8, soa=soa)


# ======================================================================== mh_reserve, then capture
@pytest.mark.parametrize("case", ["tree128_f32", "humanoid_f64"])
def test_reserve_then_capture_every_batch_class(torch_cuda, cu, case):
    """include/mecano_hip.h: after mh_reserve(max_batch) and one first call of each entry point, calls with B <= max_batch allocate nothing
    and can be captured into a graph.  The first calls here are at 64 configurations, so nothing of the big batches is planned before the
    capture: the depth-first plans of every budget a smaller batch may get (the fp32 fused pair walk of mh_rnea_aba_f32 among them) must
    come from mh_reserve.  Captured calls at the reserved size and at sizes of each smaller class replay to the results of eager calls on
    another model of the same robot, bit for bit, on the captured inputs and on new ones."""
    torch = torch_cuda
    from mecano_amd import _lib
    if case == "tree128_f32":
        rb, dt, mx = robot("tree128"), torch.float32, 131072
        sizes = (8192 + 36, 2 * cu * 64 + 1, mx)
        calls = [(n, soa) for n in ("rnea_aba", "rnea", "aba") for soa in (False, True)]
    else:
        rb, dt, mx = robot("humanoid"), torch.float64, 4 * cu * 64 + 37
        sizes = (1000, cu * 64 + 1, 2 * cu * 64 + 37, mx)
        calls = [(n, False) for n in ("rnea_aba", "rnea", "aba", "crba")]
    hm, ref = rb.model(), rb.model()
    hm.reserve(mx)
    small = rb.rows.device(torch, 64, dt)
    for name, soa in calls:
        invoke(torch, hm, name, 64, [small[k] for k in INPUTS[name]], soa)
    s = torch.cuda.Stream()
    bound = []
    with torch.cuda.stream(s):
        for B in sizes:
            ins = rb.rows.device(torch, B, dt)
            for name, soa in calls:
                bound.append((name, soa, B) + prepare(torch, hm, name, B, [ins[k] for k in INPUTS[name]], soa))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            for name, soa, B, fn, args, _keep, _outs in bound:
                _lib.check(fn(*args))
    torch.cuda.synchronize()
    other = DistinctRows(rb.sys, 512, 99)
    for replay in range(2):
        if replay:  # new inputs written into the captured buffers
            for B in sizes:
                new = other.device(torch, B, dt)
                for name, soa, b, fn, args, keep, outs in bound:
                    if b == B:
                        for x, k in zip(keep[0], INPUTS[name]):
                            x.copy_(new[k].t() if soa else new[k])
            torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for name, soa, B, fn, args, keep, outs in bound:
            x = [t.t().contiguous() if soa else t for t in keep[0]]  # the AoS inputs again
            want = invoke(torch, ref, name, B, x, soa)
            for (rows, guard), (wrows, _) in zip(outs, want):
                assert torch.isnan(guard).all(), (name, soa, B)
                assert torch.equal(rows, wrows), (case, name, "soa" if soa else "aos", B, replay)


def _lane_workspace_calls(torch, hm, B, ins):
    """The entry points whose kernels take `parts` waves per group of configurations, each on a workspace block of its own, bound to
    preallocated outputs: [(name, call, outputs)].  call() issues the entry point on the current stream."""
    from mecano_amd import _lib
    lib = _lib.load()
    q, qd, qdd, tau = ins
    nv, nq, nj = hm.nv, hm.nq, hm.n_joints
    new = lambda *shape: torch.full((B,) + shape, float("nan"), dtype=q.dtype, device=q.device)
    targets = np.arange(16) % nj
    g, _ = hm._root(G)
    opts = lambda: ctypes.byref(hm._options(_lib.LAYOUT_AOS, stream=torch.cuda.current_stream().cuda_stream))
    p = lambda t: t.data_ptr()
    Y, H, C, A, b, com = new(nv, 10 * nj), new(nv, nv), new(nv, nv), new(6, nv), new(6), new(3)
    grav, W, Hinv, poses, jac = (new(nv), new(nv, nv)), new(16, 6, 6), new(nv, nv), new(nj, 12), (new(6 * 16, nv), new(16, 6))
    rd, ad = (new(nv), new(nv, nv), new(nv, nv)), (new(nv), new(nv, nv), new(nv, nv), new(nv, nv))
    sd = (new(nv), q.clone(), qd.clone(), new(2 * nv, 2 * nv), new(2 * nv, nv))
    return [
        ("regressor", lambda: _lib.check(lib.mh_regressor_f64(hm._h, B, p(q), p(qd), p(qdd), g, opts(), 0, p(Y))), (Y,)),
        ("crba_coriolis", lambda: _lib.check(lib.mh_crba_coriolis_f64(hm._h, B, p(q), p(qd), opts(), p(H), p(C))), (H, C)),
        ("centroidal", lambda: _lib.check(lib.mh_centroidal_f64(hm._h, B, p(q), p(qd), None, _lib.CENTROIDAL_FRAME_FIXED, opts(), p(A), p(b),
                                                                 p(com))), (A, b, com)),
        ("gravity_gradient", lambda: hm.gravity_gradient(q, G, out=grav), grav),
        ("apparent_inertia_inverse", lambda: hm.apparent_inertia_inverse(q, targets, coupled=False, out=W), (W,)),
        ("mass_matrix_inverse", lambda: hm.mass_matrix_inverse(q, out=Hinv), (Hinv,)),
        ("rnea_derivatives", lambda: hm.rnea_derivatives(q, qd, qdd, G, out=rd), rd),
        ("aba_derivatives", lambda: hm.aba_derivatives(q, qd, tau, G, out=ad), ad),
        ("step_derivatives", lambda: hm.step_derivatives(DT, q, qd, tau, G, out=sd), sd),
        ("body_poses", lambda: hm.body_poses(q, out=poses), (poses,)),
        ("geometric_jacobian", lambda: hm.geometric_jacobian(q, targets, qd=qd, convective=True, out=jac), jac),
    ]


def test_reserve_covers_every_smaller_batch_of_the_lane_workspace_kernels(torch_cuda):
    """mh_reserve(max_batch) covers every B <= max_batch, not max_batch alone: the kernels that put several waves on a group of 64
    configurations take grid * parts workspace blocks, and that product is not monotonic in the batch.  With 3 CUs (12 waves):
    B = 320 is grid 5 x 2 parts = 10 waves, B = 191 is grid 3 x 4 parts = 12.  After reserve(320) and first calls at 64, every such entry
    point is captured at 191 and at 320 -- an allocation inside the capture makes the call fail -- and replays to the bits of eager calls
    on another model of the same robot."""
    torch = torch_cuda
    rb = robot("humanoid")
    hm, ref = rb.model(MH_FAKE_CU_COUNT=3), rb.model(MH_FAKE_CU_COUNT=3)
    hm.reserve(320)
    for _name, call, _outs in _lane_workspace_calls(torch, hm, 64, rb.rows.device(torch, 64, torch.float64)):
        call()
    s = torch.cuda.Stream()
    bound = []
    with torch.cuda.stream(s):
        for B in (191, 320):
            ins = rb.rows.device(torch, B, torch.float64)
            bound += [(B, ins) + c for c in _lane_workspace_calls(torch, hm, B, ins)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            for B, _ins, _name, call, _outs in bound:
                call()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for B in (191, 320):
        ins = next(i for b, i, *_ in bound if b == B)
        eager = _lane_workspace_calls(torch, ref, B, ins)
        for _name, call, _outs in eager:
            call()
        torch.cuda.synchronize()
        want = {name: outs for name, _call, outs in eager}
        for b, _ins, name, _call, outs in bound:
            if b == B:
                for k, (got, exp) in enumerate(zip(outs, want[name])):
                    assert not torch.isnan(exp).any(), (name, B, k)
                    assert torch.equal(got, exp), (name, B, k)
