"""What mh_model_create compiles from a description (mecano_amd/csrc/mh_model_tables.h: compile_model), read on the CPU through
mh_internal_model_table: no device is needed, none is used.

Three kinds of checks.  PINNED: every table of every model below equals, bit for bit, what the statements of mh_model_create produced
before they moved into compile_model (tests/golden/model_tables.json, written once by tests/golden/make_model_tables_fixtures.py from the
moved, unchanged text) -- integer tables and doubles alike: bit-equal body constants are what keep every parity number where it is.
INVARIANTS: what the kernels rely on, restated in numpy from the description, independent of the fixture.  NO DEVICE: the error codes
and their precedence stay what tests/test_abi.py expects."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from mecano_amd import _lib
from mecano_amd import random_tools as rt
from mecano_amd.multibody import ModelDesc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGISTERED = ("arm7", "humanoid30", "tree128")
# tests/golden/model_tables_models.json: flat mh_model_desc form of the models that are not under mecano_amd/models/
STORED = ("one_revolute", "one_fixed", "chain2", "star", "every_kind_permuted", "forest2", "near_axis", "tiny_composite")
MODELS = REGISTERED + STORED

INT_TABLES = ("meta", "dof_map", "cfg_map", "engine_of", "prog", "prog_seq", "grav_zero_ofs", "grav_zero_cols", "resp_info", "minv_owner", "deriv_slot")
F64_TABLES = ("consts", "sub_mass", "inertial_parameters")
SCALARS = ("n", "nq", "nv", "n_slots", "rnea_stack", "aba_stack", "pair_stack", "aba_hand", "n_nonadjacent", "resp_slots", "resp_a_base", "resp_u_base",
           "deriv_slots", "ident_maps", "dense_maps", "q_may_be_out", "warnings")  # the order of the "scalars" table (mh_api.hip)

# the layouts the kernels' headers declare (mh_kernels.h, mh_response_kernels.h, mh_rnea_deriv_kernels.h, mh_dfs_kernels.h)
MI_PARENT, MI_TYPE, MI_DOF, MI_CFG, MI_EXT, MI_FLAGS, MI_SLOT_JP, MI_SLOT_F, MI_SLOT_VA, MI_SLOT_C, MI_SLOT_IA, MI_SLOT_LK, MI_STRIDE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 24
MF_STORE_VA = 2
MC_RB, MC_PB, MC_M, MC_H, MC_I, MC_QA, MC_OA, MC_STRIDE = 0, 9, 12, 13, 16, 34, 43, 46
RI_TIN, RI_TOUT, RI_STRIDE = 0, 1, 4
DS_BODY, DS_BRANCH = 68, 84
EV_POP, EV_LEAF, EV_LAST_CHILD, EV_BODY_SHIFT = 1, 2, 4, 8
REVOLUTE, PRISMATIC = 0, 1
NDOF = {0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}


def model_desc(name):
    if name in REGISTERED:
        return rt.modelDescFromJson(name)
    with open(os.path.join(GOLDEN, "model_tables_models.json")) as f:
        d = json.load(f)[name]
    return ModelDesc(d["n_joints"], d["nq"], d["nv"], np.array(d["parent"], dtype=np.int32), np.array(d["joint_type"], dtype=np.int32),
                     np.array(d["axis"]), np.array(d["X_before"]), np.array(d["X_com"]), np.array(d["inertia_J"]), np.array(d["inertia_mass"]),
                     np.array(d["inertia_com"]), np.array(d["dof_indices"], dtype=np.int32), np.array(d["cfg_indices"], dtype=np.int32))


def c_desc(desc, keep):
    """The description as the C struct; an array without entries (a model of fixed joints has no index maps) still gets an address."""
    d = _lib.MhModelDesc()
    d.n_joints, d.nq, d.nv = int(desc.n_joints), int(desc.nq), int(desc.nv)
    for k, dt in (("parent", np.int32), ("joint_type", np.int32), ("dof_indices", np.int32), ("cfg_indices", np.int32), ("axis", np.float64),
                  ("X_before", np.float64), ("X_com", np.float64), ("inertia_J", np.float64), ("inertia_mass", np.float64), ("inertia_com", np.float64)):
        a = np.ascontiguousarray(np.asarray(getattr(desc, k), dtype=dt).reshape(-1))
        a = a if a.size else np.zeros(1, dtype=dt)
        keep.append(a)
        setattr(d, k, a.ctypes.data_as(ctypes.c_void_p))
    return d


def table_status(lib, d, name, dtype=np.uint8):
    size = ctypes.c_size_t(0)
    st = lib.mh_internal_model_table(ctypes.byref(d), name.encode(), None, 0, ctypes.byref(size))
    if st != 0:
        return st, None
    out = np.zeros(size.value // np.dtype(dtype).itemsize, dtype=dtype)
    st = lib.mh_internal_model_table(ctypes.byref(d), name.encode(), out.ctypes.data_as(ctypes.c_void_p), out.nbytes, ctypes.byref(size))
    assert size.value == out.nbytes
    return st, out


def tables_of(lib, desc):
    """Every member of ModelTables of a description, by name."""
    keep = []
    d = c_desc(desc, keep)
    out = {}
    for name, dtype in [("scalars", np.int32), ("nonleaf_fraction", np.float64), ("topo_key", np.uint8), ("warning_text", np.uint8)] \
            + [(t, np.int32) for t in INT_TABLES] + [(t, np.float64) for t in F64_TABLES]:
        st, a = table_status(lib, d, name, dtype)
        assert st == 0, (name, lib.mh_last_error().decode())
        out[name] = a
    return out


def digest(t):
    """The form of a model's tables that tests/golden/model_tables.json keeps: hashes of the tables' bytes, the small things verbatim."""
    doc = {"scalars": dict(zip(SCALARS, (int(x) for x in t["scalars"]))), "nonleaf_fraction": float(t["nonleaf_fraction"][0]).hex(),
           "topo_key": t["topo_key"].tobytes().decode(), "warning_text": t["warning_text"].tobytes().decode(), "sha256": {}}
    assert len(t["scalars"]) == len(SCALARS)
    for name in INT_TABLES + F64_TABLES:
        doc["sha256"][name] = hashlib.sha256(t[name].tobytes()).hexdigest()
    return doc


@pytest.fixture(scope="module")
def compiled(hip_lib):
    """name -> (description, tables): compiled once, shared, read-only."""
    out = {}
    for name in MODELS:
        desc = model_desc(name)
        tables = tables_of(hip_lib, desc)
        for a in tables.values():
            a.setflags(write=False)
        out[name] = (desc, tables)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "model_tables.json")) as f:
        return json.load(f)["models"]


# ------------------------------------------------------------------------------------------------ pinned to the parent
@pytest.mark.parametrize("name", MODELS)
def test_tables_equal_the_ones_model_creation_made_before_the_move(compiled, golden, name):
    got, want = digest(compiled[name][1]), golden[name]
    for key in ("scalars", "nonleaf_fraction", "topo_key", "warning_text"):
        assert got[key] == want[key], f"{name}: {key}: {got[key]!r} != {want[key]!r}"
    assert sorted(got["sha256"]) == sorted(want["sha256"])
    for table in INT_TABLES + F64_TABLES:
        assert got["sha256"][table] == want["sha256"][table], f"{name}: table {table} differs from the pinned one"


def test_the_models_cover_the_cases_they_are_here_for(compiled):
    s = {name: dict(zip(SCALARS, (int(x) for x in compiled[name][1]["scalars"]))) for name in MODELS}
    assert s["one_fixed"]["nv"] == 0 and s["one_fixed"]["nq"] == 0 and s["one_fixed"]["n_slots"] >= 1
    assert s["every_kind_permuted"]["dense_maps"] == 0 and s["every_kind_permuted"]["ident_maps"] == 0
    assert sorted(set(compiled["every_kind_permuted"][0].joint_type.tolist())) == [0, 1, 2, 3, 4, 5]
    assert (compiled["forest2"][0].parent < 0).sum() == 2
    assert s["near_axis"]["warnings"] == 1 and "within 1e-7" in compiled["near_axis"][1]["warning_text"].tobytes().decode()
    assert s["tiny_composite"]["warnings"] == 2 and "1e-7" in compiled["tiny_composite"][1]["warning_text"].tobytes().decode()
    assert s["arm7"]["ident_maps"] == 1 and s["arm7"]["q_may_be_out"] == 1 and s["humanoid30"]["q_may_be_out"] == 0
    # the star: one body with three children, two of them leaves
    parent = compiled["star"][0].parent
    kids = [int(c) for c in np.flatnonzero(parent == 0)]
    assert len(kids) == 3 and sum(1 for c in kids if not (parent == c).any()) == 2


# ------------------------------------------------------------------------------------------------ invariants, restated in numpy
class Tree:
    """The engine-order view of a compiled model, from its body records and the description alone."""

    def __init__(self, desc, t):
        self.desc, self.t = desc, t
        self.n = int(desc.n_joints)
        self.meta = t["meta"].reshape(self.n, MI_STRIDE)
        self.parent = self.meta[:, MI_PARENT]
        self.type = self.meta[:, MI_TYPE]
        self.ext = self.meta[:, MI_EXT]
        self.ndof = np.array([NDOF[int(k)] for k in self.type])
        self.edofo = np.concatenate([[0], np.cumsum(self.ndof)])
        self.children = [[int(c) for c in np.flatnonzero(self.parent == e)] for e in range(self.n)]
        self.scalars = dict(zip(SCALARS, (int(x) for x in t["scalars"])))

    def ancestors_and_self(self, e):
        out = []
        while e >= 0:
            out.append(e)
            e = int(self.parent[e])
        return out

    def related(self, a, b):
        return a in self.ancestors_and_self(b) or b in self.ancestors_and_self(a)


@pytest.fixture(scope="module")
def trees(compiled):
    return {name: Tree(*compiled[name]) for name in MODELS}


@pytest.mark.parametrize("name", MODELS)
def test_engine_order_and_index_maps(trees, name):
    T = trees[name]
    desc, t = T.desc, T.t
    assert all(-1 <= T.parent[e] < e for e in range(T.n))  # parents first
    assert sorted(T.ext.tolist()) == list(range(T.n))
    assert np.array_equal(t["engine_of"][T.ext], np.arange(T.n))
    assert np.array_equal(T.type, np.asarray(desc.joint_type)[T.ext])
    caller_parent = np.asarray(desc.parent)[T.ext]
    assert np.array_equal(T.parent, np.where(caller_parent < 0, -1, t["engine_of"][np.maximum(caller_parent, 0)]))
    assert np.array_equal(T.meta[:, MI_DOF], T.edofo[:-1])
    # the maps are the description's, joint by joint in engine order
    dofo = np.concatenate([[0], np.cumsum([NDOF[int(k)] for k in desc.joint_type])])
    want = [int(x) for e in range(T.n) for x in np.asarray(desc.dof_indices)[dofo[T.ext[e]]:dofo[T.ext[e] + 1]]]
    assert t["dof_map"].tolist() == (want or [0])


@pytest.mark.parametrize("name", MODELS)
def test_euler_tour_decides_subtree_membership(trees, name):
    T = trees[name]
    info = T.t["resp_info"].reshape(T.n, RI_STRIDE)
    tin, tout = info[:, RI_TIN], info[:, RI_TOUT]
    assert sorted(np.concatenate([tin, tout]).tolist()) == list(range(2 * T.n))
    under = np.zeros((T.n, T.n), dtype=bool)  # under[j, x]: x in the subtree of j
    for x in range(T.n):
        under[T.ancestors_and_self(x), x] = True
    assert np.array_equal(under, (tin[:, None] <= tin[None, :]) & (tout[None, :] <= tout[:, None]))


@pytest.mark.parametrize("name", MODELS)
def test_gravity_gradient_zero_pattern(trees, name):
    T = trees[name]
    nv, dof_map = T.scalars["nv"], T.t["dof_map"]
    ofs, cols = T.t["grav_zero_ofs"], T.t["grav_zero_cols"]
    assert len(ofs) == T.n + 2 and ofs[0] == 0
    owned = set(int(dof_map[k]) for k in range(T.edofo[T.n]))
    unowned = [r for r in range(nv) if r not in owned]
    for e in range(T.n):
        got = cols[ofs[e]:ofs[e + 1]].tolist()
        want = []
        if T.ndof[e]:
            want = [int(dof_map[k]) for b in range(T.n) if not T.related(e, b) for k in range(T.edofo[b], T.edofo[b + 1])] + unowned
        assert len(got) == len(set(got)) and set(got) == set(want), (name, e)
    assert cols[ofs[T.n]:ofs[T.n + 1]].tolist() == unowned
    assert len(cols) == max(1, int(ofs[T.n + 1]))


@pytest.mark.parametrize("name", MODELS)
def test_dof_owners_invert_the_dof_map(trees, name):
    T = trees[name]
    owner = T.t["minv_owner"]
    want = np.full(max(1, T.scalars["nv"]), -1)
    for e in range(T.n):
        for k in range(T.ndof[e]):
            want[T.t["dof_map"][T.edofo[e] + k]] = 8 * e + k
    assert np.array_equal(owner, want)


def _disjoint_below(ranges, limit):
    ranges = sorted(r for r in ranges if r[1] > r[0])
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])) and all(0 <= a and b <= limit for a, b in ranges)


@pytest.mark.parametrize("name", MODELS)
def test_slot_plans_do_not_overlap(trees, name):
    T = trees[name]
    ranges = []
    for e in range(T.n):
        mi, branch = T.meta[e], bool(T.meta[e, MI_FLAGS] & MF_STORE_VA)
        assert branch == any(c != e + 1 for c in T.children[e])
        for field, size in ((MI_SLOT_JP, 2 if T.type[e] == REVOLUTE else 0), (MI_SLOT_F, 8), (MI_SLOT_C, 6), (MI_SLOT_VA, 12 if branch else 0),
                            (MI_SLOT_IA, 40 if branch else 0), (MI_SLOT_LK, 27 if T.ndof[e] >= 3 else 0)):
            ranges.append((int(mi[field]), int(mi[field]) + size))
    assert _disjoint_below(ranges, T.scalars["n_slots"])
    ds = T.t["deriv_slot"]
    sizes = [DS_BRANCH if T.meta[e, MI_FLAGS] & MF_STORE_VA else DS_BODY for e in range(T.n)]
    assert _disjoint_below([(int(ds[e]), int(ds[e]) + sizes[e]) for e in range(T.n)], T.scalars["deriv_slots"])
    assert 0 <= T.scalars["resp_a_base"] <= T.scalars["resp_u_base"] <= T.scalars["resp_slots"]


@pytest.mark.parametrize("which", ["prog", "prog_seq"])
@pytest.mark.parametrize("name", MODELS)
def test_event_programs(trees, name, which):
    T = trees[name]
    prog = T.t[which]
    body, is_pop = prog >> EV_BODY_SHIFT, (prog & EV_POP) != 0
    assert len(prog) == 2 * T.n
    visit_at, pop_at = np.full(T.n, -1), np.full(T.n, -1)
    for i in range(len(prog)):
        at = pop_at if is_pop[i] else visit_at
        assert at[body[i]] == -1, "a body is visited once and popped once"
        at[body[i]] = i
    assert (visit_at >= 0).all() and (pop_at >= 0).all()
    for e in range(T.n):
        assert visit_at[e] < pop_at[e]
        for c in T.children[e]:
            assert visit_at[e] < visit_at[c] and pop_at[c] < pop_at[e]
        # EV_LEAF: exactly the pops that directly follow their visit
        assert bool(prog[pop_at[e]] & EV_LEAF) == (pop_at[e] == visit_at[e] + 1)
        if T.children[e]:
            assert sum(1 for c in T.children[e] if prog[pop_at[c]] & EV_LAST_CHILD) == 1
            if which == "prog":  # the leaves behind the children with subtrees
                walked = sorted(T.children[e], key=lambda c: visit_at[c])
                leaf = [not T.children[c] for c in walked]
                assert leaf == sorted(leaf)
    for r in np.flatnonzero(T.parent < 0):
        assert not prog[pop_at[r]] & EV_LAST_CHILD


@pytest.mark.parametrize("name", MODELS)
def test_body_constants(trees, name):
    T = trees[name]
    desc = T.desc
    c = T.t["consts"].reshape(T.n, MC_STRIDE)
    axis, Xb, Xc = np.asarray(desc.axis).reshape(-1, 3), np.asarray(desc.X_before).reshape(-1, 12), np.asarray(desc.X_com).reshape(-1, 12)
    J, mass, com = np.asarray(desc.inertia_J).reshape(-1, 3, 3), np.asarray(desc.inertia_mass).reshape(-1), np.asarray(desc.inertia_com).reshape(-1, 3)
    for e in range(T.n):
        i = int(T.ext[e])
        one_dof = T.type[e] in (REVOLUTE, PRISMATIC)
        Rb = c[e, MC_RB:MC_RB + 9].reshape(3, 3)
        assert np.abs(Rb @ Rb.T - np.eye(3)).max() <= 1e-14, (name, e)
        if e > 0 and T.parent[e] == e - 1 and T.type[e - 1] in (REVOLUTE, PRISMATIC):  # the first child of a 1-DoF joint is x-aligned
            assert c[e, MC_PB + 1] == 0.0 and c[e, MC_PB + 2] == 0.0, (name, e)
        # the canonical frame: its z axis is the joint's axis, its origin lies on it (other joints: Mecano's after-joint frame itself)
        Q, O = c[e, MC_QA:MC_QA + 9].reshape(3, 3), c[e, MC_OA:MC_OA + 3]
        assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-14 and np.linalg.det(Q) > 0
        if one_dof:
            k = axis[i] / np.linalg.norm(axis[i])
            assert np.abs(Q[:, 2] - k).max() <= 1e-15 and np.abs(np.cross(O, k)).max() <= 1e-15 * max(1.0, np.abs(O).max())
        else:
            assert np.array_equal(Q, np.eye(3)) and not O.any()
        # mass, first moment and rotational inertia about that origin, from the description
        Rc, pc = Xc[i, :9].reshape(3, 3), Xc[i, 9:]
        Js = 0.5 * (J[i] + J[i].T)
        r = Rc @ com[i]                    # centre of mass from the body-fixed origin, after-joint axes
        s = r + pc - O                     # ... from the canonical origin
        I_com = Rc @ Js @ Rc.T - mass[i] * (r @ r * np.eye(3) - np.outer(r, r))
        I_O = Q.T @ (I_com + mass[i] * (s @ s * np.eye(3) - np.outer(s, s))) @ Q
        h = Q.T @ (mass[i] * s)
        assert c[e, MC_M] == mass[i]
        assert np.abs(c[e, MC_H:MC_H + 3] - h).max() <= 1e-12 * max(np.abs(h).max(), 1e-300), (name, e)
        got = c[e, MC_I:MC_I + 6]
        want = np.array([I_O[0, 0], I_O[0, 1], I_O[0, 2], I_O[1, 1], I_O[1, 2], I_O[2, 2]])
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, e)


# ------------------------------------------------------------------------------------------------ without a device
def test_error_codes_and_their_precedence_without_a_device(hip_lib):
    """tests/test_abi.py's good and bad descriptions: mh_model_create answers as it did (description errors and MH_ERR_BAD_AXIS before
    MH_ERR_NO_DEVICE), and the tables' entry point gives the description's own code for each, MH_OK for the good one."""
    from test_abi import _chain_desc, _create

    def both(desc):
        keep = []
        st, _ = table_status(hip_lib, c_desc(desc, keep), "meta", np.int32)
        return _create(hip_lib, desc)[0], st

    assert both(_chain_desc()) in ((0, 0), (7, 0))
    bad = _chain_desc()
    bad.joint_type = bad.joint_type.copy()
    bad.joint_type[2] = 9
    assert both(bad) == (3, 3)  # MH_ERR_UNSUPPORTED_JOINT
    bad = _chain_desc()
    bad.parent = bad.parent.copy()
    bad.parent[1], bad.parent[2] = 2, 1
    assert both(bad) == (4, 4)  # MH_ERR_LOOP_CLOSURE
    bad = _chain_desc()
    bad.parent = bad.parent.copy()
    bad.parent[3] = 17
    assert both(bad) == (5, 5)  # MH_ERR_BAD_TOPOLOGY
    bad = _chain_desc()
    bad.axis = bad.axis.copy()
    bad.axis[3:6] *= 1.5
    assert both(bad) == (6, 6)  # MH_ERR_BAD_AXIS
    assert "not a unit vector" in hip_lib.mh_last_error().decode()
    bad = _chain_desc()
    bad.dof_indices = bad.dof_indices.copy()
    bad.dof_indices[1] = bad.dof_indices[0]
    assert both(bad) == (5, 5) and "dof_indices" in hip_lib.mh_last_error().decode()
    # the entry point's own arguments
    keep = []
    d = c_desc(_chain_desc(), keep)
    size = ctypes.c_size_t(0)
    assert hip_lib.mh_internal_model_table(ctypes.byref(d), b"no_such_table", None, 0, ctypes.byref(size)) == 1
    small = np.zeros(1, dtype=np.int32)
    assert hip_lib.mh_internal_model_table(ctypes.byref(d), b"meta", small.ctypes.data_as(ctypes.c_void_p), small.nbytes, ctypes.byref(size)) == 1
    assert size.value == 5 * MI_STRIDE * 4 and small[0] == 0
    assert hip_lib.mh_internal_model_table(None, b"meta", None, 0, ctypes.byref(size)) == 1
