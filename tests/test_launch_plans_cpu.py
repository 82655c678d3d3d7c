"""The launch planners (mecano_amd/csrc/mh_launch_plans.h: dfs_frames, dfs_choose, dfs_geometry, split_rt_plan, split_rt_records,
split_rt_shape, the lane-workspace arithmetic, the frame list and the scratch of the constrained and the contact dynamics), read on the CPU
through mh_internal_launch_plan: no device is needed, none is used.

PINNED: every plan below equals, word for word, what the statements of dfs_plan, split_rt_plan, split_rt_upload_meta, dfs_choose, dfs_setup
and launch_split_rt produced before they moved out of mh_api.hip (tests/golden/launch_plans.json, written by
tests/golden/make_launch_plan_fixtures.py from the moved, unchanged text).  INVARIANTS: what the kernels and mh_reserve rely on, restated
in numpy from the description and the model's body records, independent of the fixture."""
import ctypes
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

from test_model_tables_cpu import (GOLDEN, MODELS, MI_PARENT, MI_TYPE, MI_FLAGS, MI_SLOT_JP, MI_SLOT_F, MI_SLOT_VA, MI_SLOT_C, MI_SLOT_IA, MI_SLOT_LK,
                                   MI_STRIDE, SCALARS, c_desc, model_desc, table_status)

# two branching trees of revolute joints, as rev14 of tests/test_gpu_aliasing.py: (seed, joints)
REVOLUTE_TREES = {"rev14": (14, 14), "rev23": (23, 23)}
SPLIT_MODELS = MODELS + tuple(REVOLUTE_TREES)
CHOICE_MODELS = ("humanoid30", "tree128")

BUDGETS = (0, 9, 24, 48, 60, 80, "stack")  # "stack": the model's full stack of the algorithm
STACK_OF_ALGO = ("rnea_stack", "aba_stack", "pair_stack")
CHOICE_CUS = (1, 3, 256)
CHOICE_B = (1, 64, 357, 8192, 98304, 196608, 262144, 393216, 1048576)
# (algo, elem, aos, pair): the row windows are the inverse dynamics' on AoS rows, the fused pair walk is fp32 forward dynamics
CHOICE_CALLS = tuple((0, elem, aos, 0) for elem in (4, 8) for aos in (0, 1)) + tuple((1, elem, 0, 0) for elem in (4, 8)) + ((1, 4, 0, 1),)
CHOICE_PLACE = (-1, 0, 1, 2)
CHOICE_BUDGET = (-1, 48)
CHOICE_WORDS = ("win", "per_cu", "budget", "hand", "b_win", "slot_bytes", "hand_lds", "occ3", "lds_slots", "glb_slots", "glb_frames", "lds", "geo_per_cu", "grid",
                "gslots", "mode")
# (elem, algo, pair) of a run-time tree-split launch: the pair call is the fp64 one
SHAPE_CALLS = tuple((elem, algo, 0) for elem in (4, 8) for algo in (0, 1, 2)) + ((8, 1, 1),)

# the layouts the kernels' headers declare (mh_kernels.h, mh_dfs_kernels.h, mh_split_kernels.h)
MI_NCH, MI_DFS_R, MI_DFS_A, MI_HAND, MI_PFR_R, MI_PVA_R, MI_PFR_A, MI_PV_A, MI_PACC_A = 12, 13, 14, 15, 16, 17, 18, 19, 20
MF_PARENT_ADJ = 1
DFS_LDS = 1 << 20
SPLIT_WAVES, SPLIT_MAX_SEG, SPLIT_LDS_MARGIN = 4, 16, 48
SLOT_FIELDS = (MI_SLOT_JP, MI_SLOT_F, MI_SLOT_VA, MI_SLOT_C, MI_SLOT_IA, MI_SLOT_LK, MI_HAND)


def jx_slots(t):
    return {0: 2, 1: 1, 2: 12, 3: 0, 4: 12, 5: 12}[int(t)]


def frame_slots(algo, t, nch):
    if nch == 0:
        return 0
    rnea = 6 + jx_slots(t) + (12 if nch >= 2 else 0)
    aba = 12 + jx_slots(t) + (33 if nch >= 2 else 0)
    return (rnea, aba, aba + 6 + (6 if nch >= 2 else 0))[algo]


def any_model_desc(name):
    if name in REVOLUTE_TREES:
        from mecano_amd import random_tools as rt
        from mecano_amd.multibody import MultiBodySystem
        seed, n = REVOLUTE_TREES[name]
        joints = rt.nextJointTree(np.random.default_rng(seed), n, ("revolute",))
        return MultiBodySystem.toMultiBodySystemInput(joints[0].getPredecessor()).toModelDesc()
    return model_desc(name)


class Planner:
    """A description, its body records and scalars, and the planners on it."""

    def __init__(self, lib, name):
        self.lib, self.name, self.keep = lib, name, []
        self.d = c_desc(any_model_desc(name), self.keep)
        st, meta = table_status(lib, self.d, "meta", np.int32)
        assert st == 0
        st, scalars = table_status(lib, self.d, "scalars", np.int32)
        assert st == 0
        self.scalars = dict(zip(SCALARS, (int(x) for x in scalars)))
        self.n = self.scalars["n"]
        self.meta = meta.reshape(self.n, MI_STRIDE)
        self.meta.setflags(write=False)
        self.parent, self.type, self.nch = self.meta[:, MI_PARENT], self.meta[:, MI_TYPE], self.meta[:, MI_NCH]
        self.children = [[int(c) for c in np.flatnonzero(self.parent == e)] for e in range(self.n)]
        st, self.engine_of = table_status(lib, self.d, "engine_of", np.int32)  # caller's joint -> engine index
        assert st == 0

    def status(self, plan, *params):
        p = (ctypes.c_int64 * max(1, len(params)))(*params)
        size = ctypes.c_size_t(0)
        st = self.lib.mh_internal_launch_plan(ctypes.byref(self.d), plan.encode(), p, len(params), None, 0, ctypes.byref(size))
        if st != 0:
            return st, None
        out = np.zeros(size.value // 4, dtype=np.int32)
        st = self.lib.mh_internal_launch_plan(ctypes.byref(self.d), plan.encode(), p, len(params), out.ctypes.data_as(ctypes.c_void_p), out.nbytes, ctypes.byref(size))
        assert size.value == out.nbytes
        return st, out

    def plan(self, plan, *params):
        st, out = self.status(plan, *params)
        assert st == 0, (self.name, plan, params, self.lib.mh_last_error().decode())
        return out

    def budget(self, algo, b):
        return self.scalars[STACK_OF_ALGO[algo]] if b == "stack" else b

    def frames(self, algo, b, greedy):
        w = self.plan("dfs_frames", algo, self.budget(algo, b), greedy)
        return {"lds_slots": int(w[0]), "glb_slots": int(w[1]), "glb_frames": int(w[2]), "meta": w[3:].reshape(self.n, MI_STRIDE)}

    def split(self):
        w = self.plan("split_rt")
        out = dict(zip(("usable", "n_trunk", "n_limbs", "slots", "est", "total"), (int(x) for x in w[:6])))
        out["n_seg"] = [int(x) for x in w[6:6 + SPLIT_WAVES]]
        names = ("trunk_list", "seg", "xl_ofs", "xl", "patches")
        sizes, at = w[6 + SPLIT_WAVES:6 + SPLIT_WAVES + len(names)], 6 + SPLIT_WAVES + len(names)
        for nm, size in zip(names, sizes):
            out[nm] = w[at:at + size]
            at += size
        assert at == len(w)
        return out

    def records(self, k):
        w = self.plan("split_rt_records", k)
        return {"lds_slots": int(w[0]), "meta": w[3:3 + w[1]].reshape(self.n, MI_STRIDE), "xl": w[3 + w[1]:3 + w[1] + w[2]]}

    def choices(self, cu, place, budget):
        """[B][call] -> the words of dfs_choice, for one CU count and one pair of switches"""
        return np.array([[self.plan("dfs_choice", cu, algo, elem, B, aos, pair, place, budget) for algo, elem, aos, pair in CHOICE_CALLS] for B in CHOICE_B])

    def shapes(self, cu):
        return np.array([[self.plan("split_rt_shape", cu, elem, algo, B, pair) for elem, algo, pair in SHAPE_CALLS] for B in CHOICE_B])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def frames_digest(P):
    out = {}
    for algo, b, greedy in itertools.product((0, 1, 2), BUDGETS, (0, 1)):
        f = P.frames(algo, b, greedy)
        out[f"algo{algo}/budget_{b}/greedy{greedy}"] = {"slots": [P.budget(algo, b), f["lds_slots"], f["glb_slots"], f["glb_frames"]], "meta": sha(f["meta"])}
    return out


def split_digest(P):
    s = P.split()
    out = {k: v for k, v in s.items() if not isinstance(v, np.ndarray)}
    out["sha256"] = {k: sha(v) for k, v in s.items() if isinstance(v, np.ndarray)}
    if s["usable"]:
        out["records"] = []
        for k in range(3):
            r = P.records(k)
            out["records"].append({"lds_slots": r["lds_slots"], "meta": sha(r["meta"]), "xl": sha(r["xl"])})
        out["shapes"] = {f"cu{cu}": sha(P.shapes(cu)) for cu in CHOICE_CUS}
    return out


def choice_digest(P):
    out = {"default_256": P.choices(256, -1, -1).reshape(len(CHOICE_B) * len(CHOICE_CALLS), -1).tolist(), "sha256": {}}
    for cu, place, budget in itertools.product(CHOICE_CUS, CHOICE_PLACE, CHOICE_BUDGET):
        out["sha256"][f"cu{cu}/place{place}/budget{budget}"] = sha(P.choices(cu, place, budget))
    return out


@pytest.fixture(scope="module")
def planners(hip_lib):
    return {name: Planner(hip_lib, name) for name in SPLIT_MODELS}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "launch_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def frame_plans(planners):
    """(model, algo, budget, greedy) -> frame plan: made once, shared, read-only."""
    out = {}
    for name in MODELS:
        for algo, b, greedy in itertools.product((0, 1, 2), BUDGETS, (0, 1)):
            out[name, algo, b, greedy] = planners[name].frames(algo, b, greedy)
    return out


# ------------------------------------------------------------------------------------------------ pinned to the parent
@pytest.mark.parametrize("name", MODELS)
def test_frame_placement_equals_the_one_before_the_move(planners, golden, name):
    got, want = frames_digest(planners[name]), golden["frames"][name]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], f"{name}: {key}: {got[key]} != {want[key]}"


@pytest.mark.parametrize("name", SPLIT_MODELS)
def test_tree_split_and_record_sets_equal_the_ones_before_the_move(planners, golden, name):
    got, want = split_digest(planners[name]), golden["split"][name]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], f"{name}: {key}: {got[key]} != {want[key]}"


@pytest.mark.parametrize("name", CHOICE_MODELS)
def test_launch_choice_and_geometry_equal_the_ones_before_the_move(planners, golden, name):
    got, want = choice_digest(planners[name]), golden["choice"][name]
    rows = [(B, call) for B in CHOICE_B for call in CHOICE_CALLS]
    for row, g, w in zip(rows, got["default_256"], want["default_256"]):
        assert g == w, f"{name}: B, (algo, elem, aos, pair) = {row}: {dict(zip(CHOICE_WORDS, g))} != {dict(zip(CHOICE_WORDS, w))}"
    assert got["sha256"] == want["sha256"]


def test_the_cases_cover_what_they_are_here_for(planners, frame_plans):
    # tree128 at 48 / 80 slots: the knapsack and the leaves-upwards rule choose different homes
    for algo, b in ((1, 48), (2, 80)):
        assert not np.array_equal(frame_plans["tree128", algo, b, 0]["meta"], frame_plans["tree128", algo, b, 1]["meta"])
    # every kernel build of the walks: all in LDS, all global, both
    modes = {(f["glb_frames"] == 0, f["lds_slots"] == 0) for (name, *_), f in frame_plans.items() if name == "tree128"}
    assert modes == {(True, False), (False, True), (False, False)}
    assert all(planners[name].split()["usable"] for name in REVOLUTE_TREES)


# ------------------------------------------------------------------------------------------------ frame homes, restated
def homes_of(P, algo, f):
    """frame size, home (LDS?) and offset of every body, from the slot codes of a frame plan"""
    code = f["meta"][:, MI_DFS_R if algo == 0 else MI_DFS_A]
    frame = np.array([frame_slots(algo, P.type[e], P.nch[e]) for e in range(P.n)])
    return frame, (code & DFS_LDS) != 0, code & (DFS_LDS - 1), code


def ancestors(P, e):
    out = []
    e = int(P.parent[e])
    while e >= 0:
        out.append(e)
        e = int(P.parent[e])
    return out


@pytest.mark.parametrize("name", MODELS)
def test_frames_keep_the_budget_on_every_path_and_their_codes_add_up(planners, frame_plans, name):
    P = planners[name]
    for algo, b, greedy in itertools.product((0, 1, 2), BUDGETS, (0, 1)):
        f, budget, where = frame_plans[name, algo, b, greedy], P.budget(algo, b), (name, algo, b, greedy)
        frame, home, off, code = homes_of(P, algo, f)
        assert not home[frame == 0].any(), where  # a leaf has no frame
        lds_end, glb_end = [0], [0]
        for e in range(P.n):
            up = ancestors(P, e)
            # the live frames of a walk are one root-to-leaf path: the LDS-homed ones of every path fit the budget
            assert sum(frame[a] for a in up + [e] if home[a]) <= budget, where
            # a body's offset: the frames of its ancestors in the same home
            assert off[e] == sum(frame[a] for a in up if home[a] == home[e]), where
            if frame[e] > 0:
                (lds_end if home[e] else glb_end).append(int(off[e] + frame[e]))
        assert f["lds_slots"] == max(lds_end) and f["glb_slots"] == max(6, max(glb_end)), where
        assert f["glb_frames"] == int(((frame > 0) & ~home).sum()), where
        assert (f["glb_frames"] == 0) == (not ((frame > 0) & ~home).any())
        # the parent's slots in a body's own record: the parent's code plus the constants the kernels add
        want = np.array(P.meta)
        want[:, MI_DFS_R if algo == 0 else MI_DFS_A] = code
        for e in range(P.n):
            pe = int(P.parent[e])
            if pe < 0:
                continue
            pj = jx_slots(P.type[pe])
            if algo == 0:
                want[e, MI_PFR_R], want[e, MI_PVA_R] = code[pe], code[pe] + 6 + pj
            else:
                want[e, MI_PFR_A], want[e, MI_PV_A], want[e, MI_PACC_A] = code[pe], code[pe] + 12 + pj, code[pe] + 18 + pj
            if algo == 2:
                pa = frame_slots(1, P.type[pe], P.nch[pe])
                want[e, MI_PFR_R], want[e, MI_PVA_R] = code[pe] + pa, code[pe] + pa + 6
        assert np.array_equal(f["meta"], want), where  # ... and nothing else of the records changes


def worth_of(P, algo):
    """What a frame in LDS saves, in slot accesses per configuration (mh_launch_plans.h, dfs_frames)"""
    worth = np.zeros(P.n, dtype=np.int64)
    for e in range(P.n):
        k, jx = int(P.nch[e]), jx_slots(P.type[e])
        in_frame = max(0, sum(1 for c in P.children[e] if P.nch[c] > 0) - 1)
        if k == 0:
            continue
        if algo == 0:
            worth[e] = 2 * (6 + jx) if k == 1 else (6 + jx + 12) + (k - 1) * 12 + 6 + in_frame * 12 + (6 + jx)
        else:
            idn = 6 if algo == 2 else 0
            acc = 27 + idn
            through = acc + (in_frame - 1) * 2 * acc + acc if in_frame > 0 else 0
            worth[e] = 2 * (6 + jx) + 2 * idn if k == 1 else (12 + jx + 6 + idn) + (k - 1) * (12 + idn) + through + (12 + jx)
    return worth


@pytest.mark.parametrize("name", [m for m in MODELS if m not in ("humanoid30", "tree128")])
def test_knapsack_saves_what_a_brute_force_over_all_home_sets_saves(planners, frame_plans, name):
    P = planners[name]
    assert P.n <= 8
    paths = [[e] + ancestors(P, e) for e in range(P.n) if not P.children[e]]
    for algo, b in itertools.product((0, 1, 2), BUDGETS):
        budget, worth = P.budget(algo, b), worth_of(P, algo)
        frame = np.array([frame_slots(algo, P.type[e], P.nch[e]) for e in range(P.n)])
        framed = [e for e in range(P.n) if frame[e] > 0]
        best = 0
        for r in range(len(framed) + 1):
            for homes in itertools.combinations(framed, r):
                if all(sum(frame[a] for a in path if a in homes) <= budget for path in paths):
                    best = max(best, int(sum(worth[e] for e in homes)))
        for greedy in (0, 1):
            _, home, _, _ = homes_of(P, algo, frame_plans[name, algo, b, greedy])
            saved = int(worth[home].sum())
            # the leaves-upwards rule (greedy, and the inverse dynamics below 64 slots) may save less; the knapsack -- or every frame in LDS -- may not
            if greedy or (algo == 0 and budget < 64):
                assert saved <= best, (name, algo, b, greedy)
            else:
                assert saved == best, (name, algo, b, greedy)


# ------------------------------------------------------------------------------------------------ the tree split, restated
@pytest.mark.parametrize("name", SPLIT_MODELS)
def test_tree_split_partitions_the_tree(planners, name):
    P = planners[name]
    s = P.split()
    chain = all(len(c) <= 1 for c in P.children) and (P.parent < 0).sum() == 1
    if chain or name == "arm7":
        assert not s["usable"]
    if not s["usable"]:
        assert P.status("split_rt_records", 0)[0] == 1 and P.status("split_rt_shape", 256, 8, 0, 64, 0)[0] == 1
        return
    cnt = np.ones(P.n, dtype=np.int64)
    for e in range(P.n - 1, 0, -1):
        if P.parent[e] >= 0:
            cnt[P.parent[e]] += cnt[e]
    trunk = np.zeros(P.n, dtype=bool)
    if s["n_trunk"]:
        trunk[s["trunk_list"]] = True
    assert s["n_trunk"] == trunk.sum() and len(s["trunk_list"]) == max(1, s["n_trunk"])
    assert all(P.parent[e] < 0 or trunk[P.parent[e]] for e in np.flatnonzero(trunk))  # closed under "parent of"
    # the segments of the four waves: whole subtrees, which partition the bodies off the trunk
    seg = s["seg"].reshape(SPLIT_WAVES, SPLIT_MAX_SEG, 2)
    covered, roots = np.zeros(P.n, dtype=np.int64), []
    for w in range(SPLIT_WAVES):
        assert 0 <= s["n_seg"][w] <= SPLIT_MAX_SEG
        for r, end in seg[w, :s["n_seg"][w]]:
            assert end == r + cnt[r]
            covered[r:end] += 1
            roots.append(int(r))
        assert not seg[w, s["n_seg"][w]:].any()
    assert np.array_equal(covered, (~trunk).astype(np.int64))
    assert s["n_limbs"] == len(roots) == sum(s["n_seg"])
    assert all(P.parent[r] < 0 or trunk[P.parent[r]] for r in roots)
    # the patches: exchange slots of 27 entries for the limb roots with a parent, new (v, a) and accumulator slots for trunk bodies that
    # had none -- handed out one behind the other from the model's own slots on
    patches = s["patches"].reshape(-1, 3)
    hand = {int(e): int(v) for e, f, v in patches if f == MI_HAND}
    assert sorted(hand) == list(range(P.n))
    assert all((hand[e] >= 0) == (e in roots and P.parent[e] >= 0) for e in range(P.n))
    ranges = [(v, v + 27) for v in hand.values() if v >= 0]
    ranges += [(int(v), int(v) + 12) for e, f, v in patches if f == MI_SLOT_VA] + [(int(v), int(v) + 40) for e, f, v in patches if f == MI_SLOT_IA]
    ranges = [(P.scalars["n_slots"],) * 2] + sorted(ranges)  # (a forest split at its roots hands out none)
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] == s["slots"]
    assert len(set(v for v in hand.values() if v >= 0)) == sum(1 for r in roots if P.parent[r] >= 0)
    flags = {int(e): int(v) for e, f, v in patches if f == MI_FLAGS}
    assert all(not flags[r] & MF_PARENT_ADJ for r in roots if P.parent[r] >= 0)
    # per trunk body exactly the limbs attached to it
    assert len(s["xl_ofs"]) == s["n_trunk"] + 1 and s["xl_ofs"][0] == 0
    for k in range(s["n_trunk"]):
        got = s["xl"][s["xl_ofs"][k]:s["xl_ofs"][k + 1]].tolist()
        assert sorted(got) == sorted(hand[r] for r in roots if P.parent[r] == s["trunk_list"][k])
    assert len(s["xl"]) == max(1, int(s["xl_ofs"][-1]))
    # the record sets: the patched records, a slot LDS-coded iff it lies below the set's share
    plain = np.array(P.meta)
    for e, f, v in patches:
        plain[e, f] = v
    for k in range(3):
        r = P.records(k)
        cap = 160 * 1024 // (64 * (4 if k == 0 else 8))
        assert r["lds_slots"] == (0 if k == 2 else (s["slots"] if s["slots"] <= cap else cap - SPLIT_LDS_MARGIN))
        for got, want in ((r["meta"][:, SLOT_FIELDS], plain[:, SLOT_FIELDS]), (r["xl"], s["xl"])):
            coded = (got >= 0) & ((got & DFS_LDS) != 0)
            assert np.array_equal(np.where(coded, got & (DFS_LDS - 1), got), want)
            assert np.array_equal(coded, (want >= 0) & (want < r["lds_slots"]))
        rest = [f for f in range(MI_STRIDE) if f not in SLOT_FIELDS]
        assert np.array_equal(r["meta"][:, rest], plain[:, rest])


@pytest.mark.parametrize("name", ["humanoid30", "rev14"])
def test_split_launch_shape_is_consistent(planners, name):
    P = planners[name]
    slots, lds_slots = P.split()["slots"], [P.records(k)["lds_slots"] for k in range(3)]
    for cu in CHOICE_CUS:
        for (B, (elem, algo, pair)), (k, mode, lds, grid) in zip(itertools.product(CHOICE_B, SHAPE_CALLS), P.shapes(cu).reshape(-1, 4)):
            groups = (B + 63) // 64
            assert grid == (2 * groups if pair else max(1, min(groups, cu * (1 if (algo == 1 and elem == 8) else 2))))
            assert k in ((0 if elem == 4 else 1), 2)
            assert mode == (0 if lds_slots[k] >= slots else (1 if lds_slots[k] == 0 else 2))
            assert lds == (0 if mode == 1 else min(slots, lds_slots[k] + SPLIT_LDS_MARGIN) * 64 * elem) and lds <= 160 * 1024


# ------------------------------------------------------------------------------------------------ what mh_reserve relies on
@pytest.mark.parametrize("cu", [1, 3, 8])
def test_lane_workspace_bound_covers_every_smaller_batch_and_want(planners, cu):
    """mh_reserve sizes the lane workspace once, with lane_ws_bound(plan_launch(max_batch), max_want): no batch up to max_batch with any
    want up to max_want may need more.  Every max_batch up to 13 rounds of 64 * cu configurations, every max_want of 1..16 and 64; the
    largest need over the batches up to max_batch is a running maximum, which makes the sweep exhaustive."""
    P = planners["one_revolute"]
    wants = list(range(1, 17)) + [64]
    top = 64 * cu * 13
    need, bound = np.zeros((top + 1, len(wants)), dtype=np.int64), np.zeros((top + 1, len(wants)), dtype=np.int64)
    for B in range(1, top + 1):
        for i, want in enumerate(wants):
            block, grid, lanes, parts, need[B, i], bound[B, i] = P.plan("lane_ws", cu, B, want)
            assert block == 64 and lanes == grid * block and 1 <= parts <= want
    need_up_to_batch = np.maximum.accumulate(need, axis=0)           # ... over every B <= max_batch
    need_up_to_both = np.maximum.accumulate(need_up_to_batch, axis=1)  # ... and every want <= max_want (wants ascend)
    bad = np.argwhere(need_up_to_both[1:] > bound[1:])
    assert bad.size == 0, f"cu_count {cu}: (max_batch - 1, index of max_want) {bad[:5].tolist()}"


@pytest.mark.parametrize("name", CHOICE_MODELS)
@pytest.mark.parametrize("cu", [1, 3, 8])
def test_batches_of_one_count_of_waves_per_cu_get_the_plans_of_their_largest(planners, name, cu):
    """mh_reserve sets up the depth-first launches once per class of batches -- a count of waves per CU --, at the class's largest batch
    within max_batch: every batch of the class takes the same frame plan and kernel, and no larger a grid.  dfs_choose reads the batch
    through its count of groups of 64 alone (its first statement), so the first and the last batch of every count stand for all of it."""
    P = planners[name]
    same = [CHOICE_WORDS.index(w) for w in ("win", "per_cu", "budget", "hand_lds", "occ3", "lds_slots", "glb_slots", "glb_frames", "lds", "geo_per_cu", "gslots", "mode")]
    grid = CHOICE_WORDS.index("grid")
    for max_batch in (64 * cu * 13, 64 * cu * 5 + 37, 100):
        cache = {}

        def choice(B, call):
            if (B, call) not in cache:
                cache[B, call] = P.plan("dfs_choice", cu, call[0], call[1], B, call[2], call[3], -1, -1)
            return cache[B, call]

        groups = (max_batch + 63) // 64
        for g in range(1, groups + 1):
            wpc = (g + cu - 1) // cu
            representative = min(max_batch, wpc * cu * 64)
            for B in sorted({64 * g - 63, min(64 * g, max_batch)}):
                for call in CHOICE_CALLS:
                    got, rep = choice(B, call), choice(representative, call)
                    assert np.array_equal(got[same], rep[same]) and got[grid] <= rep[grid], (name, cu, max_batch, B, call)


# ------------------------------------------------------------------------------------------------ constraint and contact frames, their scratch
FRAME_MODELS = ("humanoid30", "one_revolute", "every_kind_permuted")
MAX_TARGETS = 8  # MH_MAX_CONSTRAINT_TARGETS = MH_MAX_CONTACT_TARGETS
BLOCKS = ("W", "rhs", "body", "wrench", "zeros", "zpose", "twist")
MIXED = ([6, 19, 12, 23], [12, 23, -1, 3])  # the lists of tests/test_gpu_contact_between.py


def frames_status(P, targets, bases, twists):
    K = len(targets)
    st, w = P.status("constraint_frames", K, *targets, *bases, twists)
    if st != 0:
        return st, None
    n_app = int(w[0])
    at = np.cumsum([1, K, K, K, n_app, len(BLOCKS), 1])
    assert at[-1] == len(w)
    tgt, base, bslot, app_joints, offsets, total = (w[a:b] for a, b in zip(at[:-1], at[1:]))
    return st, {"n_app": n_app, "tgt": tgt.tolist(), "base": base.tolist(), "bslot": bslot.tolist(), "app_joints": app_joints.tolist(),
                "offsets": dict(zip(BLOCKS, (int(x) for x in offsets))), "total": int(total[0])}


def frames(P, targets, bases, twists=0):
    st, f = frames_status(P, targets, bases, twists)
    assert st == 0, (P.name, targets, bases, P.lib.mh_last_error().decode())
    return f


def lists_of(P, K, nonroot):
    """K targets of which the first `nonroot` are held against another joint's body; a 1-joint model has no other joint."""
    if P.n == 1:
        return ([0] * K, [-1] * K) if nonroot == 0 else None
    targets = [1 + k % (P.n - 1) for k in range(K)]
    return targets, [0] * nonroot + [-1] * (K - nonroot)


def header_total(n, nv, K, n_app, twists):
    """include/mecano_hip.h: the scratch per configuration of the rooted calls, of the relative constraints, of the relative contacts"""
    if n_app == K:
        return 36 * K * K + 6 * K + 12 * n + nv
    return 36 * n_app * n_app + 18 * K + (18 if twists else 12) * n + nv


def test_frame_lists_of_the_humanoid(planners):
    P = planners["humanoid30"]
    eng = lambda joints: [-1 if j < 0 else int(P.engine_of[j]) for j in joints]
    f = frames(P, [19], [-1])
    assert (f["n_app"], f["tgt"], f["base"], f["bslot"], f["app_joints"]) == (1, eng([19]), [-1], [-1], [19])
    f = frames(P, [23], [19])
    assert (f["n_app"], f["tgt"], f["base"], f["bslot"], f["app_joints"]) == (2, eng([23]), eng([19]), [1], [23, 19])
    targets, others = list(range(3, 11)), list(range(13, 21))
    f = frames(P, targets, [-1] * 8)
    assert (f["n_app"], f["tgt"], f["base"], f["bslot"], f["app_joints"]) == (8, eng(targets), [-1] * 8, [-1] * 8, targets)
    f = frames(P, targets, others)
    assert (f["n_app"], f["tgt"], f["base"], f["bslot"], f["app_joints"]) == (16, eng(targets), eng(others), list(range(8, 16)), targets + others)
    f = frames(P, *MIXED)
    assert (f["n_app"], f["tgt"], f["base"], f["bslot"], f["app_joints"]) == (7, eng(MIXED[0]), eng(MIXED[1]), [4, 5, -1, 6], MIXED[0] + [12, 23, 3])
    f = frames(P, [6] * 4 + [19] * 4, [12] * 4 + [23] * 4)  # a base that appears twice still gets a frame per appearance
    assert f["n_app"] == 16 and f["bslot"] == list(range(8, 16)) and f["app_joints"][8:] == [12] * 4 + [23] * 4


def test_frame_lists_hold_engine_indices(planners):
    P = planners["every_kind_permuted"]
    assert not np.array_equal(P.engine_of, np.arange(P.n))  # the model is here for its permuted engine order
    targets = list(range(P.n))[:MAX_TARGETS]
    bases = [(j + 1) % P.n if k % 2 else -1 for k, j in enumerate(targets)]
    f = frames(P, targets, bases)
    assert f["tgt"] == [int(P.engine_of[j]) for j in targets]
    assert f["base"] == [-1 if b < 0 else int(P.engine_of[b]) for b in bases]
    assert f["app_joints"] == targets + [b for b in bases if b >= 0]
    assert [s for s in f["bslot"] if s >= 0] == list(range(len(targets), f["n_app"]))


@pytest.mark.parametrize("name", FRAME_MODELS)
def test_frame_lists_refuse_what_the_calls_refuse(planners, name):
    P = planners[name]
    for targets, bases in (([P.n], [-1]), ([-1], [-1]), ([0], [P.n]), ([0], [-2]), ([0], [0]), ([0, 0, 1 << 40], [-1] * 3), ([0, 0], [-1, -(1 << 40)])):
        assert frames_status(P, targets, bases, 0)[0] == 1, (targets, bases)
        assert "constraint_frames: " in P.lib.mh_last_error().decode()
    assert frames_status(P, [0], [0], 1)[0] == 1 and "is held against its own body (joint 0)" in P.lib.mh_last_error().decode()
    assert frames_status(P, [0], [-1], 0)[0] == 0
    # the parameter list itself: K, K targets, K bases, the flag
    for params in ((), (0, 0), (MAX_TARGETS + 1,) + (0,) * (2 * MAX_TARGETS + 3), (1, 0, -1), (1, 0, -1, 2), (1, 0, -1, 0, 0), (2, 0, -1, 0), (-1, 0, 0, 0)):
        assert P.status("constraint_frames", *params)[0] == 1, params
        assert "does not take these parameters" in P.lib.mh_last_error().decode()


@pytest.mark.parametrize("name", FRAME_MODELS)
def test_scratch_totals_are_the_headers_and_the_blocks_tile_them(planners, name):
    P = planners[name]
    n, nv = P.n, P.scalars["nv"]
    rooted = {}
    for K in range(1, MAX_TARGETS + 1):
        for nonroot in range(K + 1):
            lists = lists_of(P, K, nonroot)
            if lists is None:
                continue
            for twists in (0, 1):
                f = frames(P, *lists, twists)
                n_app, rel, where = f["n_app"], nonroot > 0, (name, K, nonroot, twists)
                assert n_app == K + nonroot, where
                assert f["total"] == header_total(n, nv, K, n_app, twists), where
                # the seven blocks: one behind the other from 0 to the total in some order, an unused one empty
                size = {"W": 36 * n_app * n_app, "rhs": 6 * K, "body": 6 * n, "wrench": 6 * n, "zeros": nv, "zpose": 12 * K if rel else 0,
                        "twist": 6 * n if rel and twists else 0}
                spans = sorted((f["offsets"][b], f["offsets"][b] + size[b]) for b in BLOCKS)
                assert spans[0][0] == 0 and spans[-1][1] == f["total"], where
                assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), where         # pairwise disjoint
                assert sum(e - s for s, e in spans) == f["total"], where                  # ... and no gap
                if nonroot == 0:
                    rooted[K] = f["total"]
    # mh_reserve sets the rooted form aside at the largest list: no shorter list needs more
    assert all(rooted[K] <= rooted[MAX_TARGETS] for K in rooted)


# ------------------------------------------------------------------------------------------------ the entry point's own arguments
def test_entry_point_refuses_what_it_does_not_know(planners):
    P = planners["star"]
    assert P.status("no_such_plan")[0] == 1
    assert P.status("dfs_frames", 0, 48)[0] == 1 and P.status("dfs_frames", 3, 48, 0)[0] == 1 and P.status("dfs_frames", 0, -1, 0)[0] == 1
    assert P.status("dfs_choice", 256, 0, 4, 64, 0, 1, -1, -1)[0] == 1  # the pair walk is forward dynamics in fp32
    assert "does not take these parameters" in P.lib.mh_last_error().decode()
    size = ctypes.c_size_t(0)
    small = np.zeros(1, dtype=np.int32)
    p = (ctypes.c_int64 * 3)(0, 48, 0)
    assert P.lib.mh_internal_launch_plan(ctypes.byref(P.d), b"dfs_frames", p, 3, small.ctypes.data_as(ctypes.c_void_p), small.nbytes, ctypes.byref(size)) == 1
    assert size.value == (3 + 5 * MI_STRIDE) * 4 and small[0] == 0
    assert P.lib.mh_internal_launch_plan(None, b"split_rt", None, 0, None, 0, ctypes.byref(size)) == 1
