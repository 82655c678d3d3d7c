"""Pins of the scattered-index-map builders of tests/helpers.py, and of the map handling of the four CPU checkers that read a description's
index maps themselves (kinematics, gravity gradient, joint limits, mass-matrix inverse): the checker on a scattered description and
moved inputs gives the moved result of the checker on the identity description to 1e-12 absolute (achieved: the same bits, 3e-15 where the joint-limit checker
inverts a permuted H), also with two indices of each space owned by no joint where the checker can take them.  No GPU."""
import numpy as np
import pytest

import gravity_gradient_check as gc
import joint_limits_check as jl
import kinematics_check as kc
import mass_matrix_inverse_check as mc
from helpers import (DistinctRows, UNOWNED, from_cols, from_step, from_v, from_vv, humanoid, keep_order, keep_order_step, mixed_tree,
                     quaternion_joints, relisted, scattered_maps, to_q, to_v, unowned)
from mecano_amd import random_tools as rt
from oracle.cpu_oracle import OracleModel

MODELS = {"mixed10": mixed_tree, "humanoid30": humanoid}
GRAVITY = np.array([0.3, -0.2, -9.81])
B = 5


@pytest.mark.parametrize("holes", [0, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_no_owned_entry_keeps_its_place_and_holes_lie_inside(name, holes):
    _, d0 = MODELS[name]()
    assert np.array_equal(d0.dof_indices, np.arange(d0.nv)) and np.array_equal(d0.cfg_indices, np.arange(d0.nq))  # the identity to start from
    rng = np.random.default_rng(1)
    ends = 0
    for _ in range(20):
        d, pv, pq = scattered_maps(d0, rng, holes)
        assert (d.nv, d.nq) == (d0.nv + holes, d0.nq + holes) and (d0.nv, d0.nq) == (int(MODELS[name]()[1].nv), int(MODELS[name]()[1].nq))
        assert len(set(pv.tolist())) == d0.nv and len(set(pq.tolist())) == d0.nq and pv.max() < d.nv and pq.max() < d.nq
        assert not np.any(pv == np.arange(d0.nv)) and not np.any(pq == np.arange(d0.nq))
        assert np.array_equal(d.dof_indices, pv[d0.dof_indices]) and np.array_equal(d.cfg_indices, pq[d0.cfg_indices])
        assert d.dof_indices.dtype == np.int32 and d.cfg_indices.dtype == np.int32
        assert not np.array_equal(pv[:min(len(pv), len(pq))], pq[:min(len(pv), len(pq))])  # drawn independently
        assert len(unowned(pv, d.nv)) == holes and len(unowned(pq, d.nq)) == holes
        ends += holes > 0 and np.array_equal(unowned(pv, d.nv), np.arange(d0.nv, d.nv))
    assert ends < 20  # the holes are not parked behind the owned rows


@pytest.mark.parametrize("name", list(MODELS))
def test_the_parts_of_a_quaternion_part_company(name):
    _, d0 = MODELS[name]()
    quats = quaternion_joints(d0)
    assert quats, "the model has no quaternion to split"
    if name == "mixed10":
        types = [int(t) for t in d0.joint_type]
        assert 2 in types and 4 in types and 5 in types and d0.nq != d0.nv  # floating, planar, spherical
    d, _, pq = scattered_maps(d0, np.random.default_rng(2))
    split = 0
    for _, at in quats:
        where = np.sort(np.asarray(d.cfg_indices)[at])
        split += not np.array_equal(np.diff(where), [1, 1, 1])
    assert split >= 1
    q = np.arange(d0.nq, dtype=float)[None, :]
    assert np.array_equal(to_q(q, pq, d.nq)[0, np.asarray(d.cfg_indices)], q[0, np.asarray(d0.cfg_indices)])  # every joint finds its own entries


def test_the_mixed_tree_is_well_conditioned_on_the_rows_the_device_tests_use():
    sys_, d0 = mixed_tree()
    assert sorted(set(int(t) for t in d0.joint_type)) == [0, 1, 2, 3, 4, 5] and d0.n_joints == 10
    om = OracleModel(d0)
    qs = [rt.nextState(np.random.default_rng(s), sys_, 70)[0] for s in (5, 6, 7)] + [DistinctRows(sys_, 16, 3).rows(np.arange(70))[0]]
    worst = max(np.linalg.cond(H, np.inf) for q in qs for H in om.crba(q))
    print(f"mixed tree: cond_inf(H) up to {worst:.2e}")
    assert worst < 1.0e8


@pytest.mark.parametrize("holes", [0, 2])
def test_movers_are_mutual_inverses(holes):
    _, d0 = mixed_tree()
    rng = np.random.default_rng(3)
    d, pv, pq = scattered_maps(d0, rng, holes)
    nv0, nv = d0.nv, d.nv
    x, q = rng.normal(size=(B, nv0)), rng.normal(size=(B, d0.nq))
    for src, perm, n in ((x, pv, nv), (q, pq, d.nq)):
        moved = to_v(src, perm, n)
        back, free = from_v(moved, perm)
        assert np.array_equal(back, src) and free.shape == (B, holes) and np.all(free == UNOWNED)
        assert np.array_equal(np.sort(keep_order(moved, perm), axis=1), np.sort(src, axis=1)) and not np.array_equal(keep_order(moved, perm), src)
    M = rng.normal(size=(B, nv0, nv0))
    wide = np.full((B, nv, nv), UNOWNED)
    wide[np.ix_(np.arange(B), pv, pv)] = M
    back, rows, cols = from_vv(wide, pv)
    assert np.array_equal(back, M) and rows.shape == (B, holes, nv) and cols.shape == (B, nv, holes) and np.all(rows == UNOWNED) and np.all(cols == UNOWNED)
    assert not np.array_equal(keep_order(wide, pv, (-2,))[:, :, pv], M) and not np.array_equal(keep_order(wide, pv, (-1,))[:, pv, :], M)
    J = rng.normal(size=(B, 12, nv0))
    wide = np.full((B, 12, nv), UNOWNED)
    wide[:, :, pv] = J
    back, cols = from_cols(wide, pv)
    assert np.array_equal(back, J) and np.all(cols == UNOWNED) and cols.shape == (B, 12, holes)
    p2 = np.concatenate([pv, nv + pv])
    for width, pc in ((2 * nv0, p2), (nv0, pv)):
        M = rng.normal(size=(B, 2 * nv0, width))
        wide = np.full((B, 2 * nv, width + (2 if width == 2 * nv0 else 1) * holes), UNOWNED)
        wide[np.ix_(np.arange(B), p2, pc)] = M
        back, rows, cols = from_step(wide, pv)
        assert np.array_equal(back, M) and np.all(rows == UNOWNED) and np.all(cols == UNOWNED)
        assert rows.shape[1] == 2 * holes and cols.shape[2] == (2 if width == 2 * nv0 else 1) * holes
        assert np.array_equal(keep_order_step(wide, pv, rows=False, cols=False), M)
        for r, c in ((True, False), (False, True)):
            other = keep_order_step(wide, pv, rows=r, cols=c)
            assert other.shape == M.shape and not np.array_equal(other, M)


def test_relisting_keeps_the_mechanism():
    _, d0 = humanoid()
    d, order = relisted(d0, np.random.default_rng(4))
    assert any(d.parent[k] > k for k in range(d.n_joints))  # a parent listed after its child
    inv = np.argsort(order)
    for j in range(d0.n_joints):  # joint j of the original is joint inv[j] of the copy: same kind, parent, constants and matrix rows
        k = int(inv[j])
        assert int(d.joint_type[k]) == int(d0.joint_type[j])
        assert int(d.parent[k]) == (-1 if d0.parent[j] < 0 else int(inv[d0.parent[j]]))
        assert mc.joint_dofs(d, k) == mc.joint_dofs(d0, j)
        for name, w in (("axis", 3), ("X_before", 12), ("X_com", 12), ("inertia_J", 9), ("inertia_com", 3), ("inertia_mass", 1)):
            assert np.array_equal(np.asarray(getattr(d, name)).reshape(-1, w)[k], np.asarray(getattr(d0, name)).reshape(-1, w)[j])
    assert sorted(np.asarray(d.cfg_indices).tolist()) == list(range(d0.nq))
    fl = int(inv[next(j for j in range(d0.n_joints) if int(d0.joint_type[j]) == 2)])
    assert [c for _, at in quaternion_joints(d) for c in np.asarray(d.cfg_indices)[at]] == [0, 1, 2, 3] and quaternion_joints(d)[0][0] == fl


def states(name):
    sys_, d0 = MODELS[name]()
    q, qd, _, _ = DistinctRows(sys_, 3, 7).rows(np.arange(B))
    return d0, q, qd


def same(moved_back, ref, label):
    """|difference|_inf <= 1e-12, absolute"""
    err = float(np.abs(moved_back - ref).max())
    print(f"{label}: {err:.3e} (|ref| up to {float(np.abs(ref).max()):.3g})")
    assert err <= 1.0e-12, f"{label}: {err:.3e}"


@pytest.mark.parametrize("holes", [0, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_kinematics_checker_reads_the_maps(name, holes):
    d0, q, qd = states(name)
    d, pv, pq = scattered_maps(d0, np.random.default_rng(6), holes)
    m0, m1 = kc.KinModel(d0), kc.KinModel(d)
    targets, bases = [d0.n_joints - 1, 2, 0], [-1, d0.n_joints - 2, 1]
    same(kc.body_poses(m1, to_q(q, pq, d.nq)), kc.body_poses(m0, q), "poses")
    J0, c0 = kc.geometric_jacobian(m0, q, targets, bases, None, qd)
    J1, c1 = kc.geometric_jacobian(m1, to_q(q, pq, d.nq), targets, bases, None, to_v(qd, pv, d.nv))
    same(from_cols(J1, pv)[0], J0, "J")
    same(c1, c0, "convective term")
    assert np.abs(keep_order(J1, pv) - J0).max() > 1.0e-3


@pytest.mark.parametrize("holes", [0, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_gravity_gradient_checker_reads_the_maps(name, holes):
    d0, q, _ = states(name)
    d, pv, pq = scattered_maps(d0, np.random.default_rng(7), holes)
    f = np.random.default_rng(8).uniform(-10.0, 10.0, (B, d0.n_joints, 6))
    tau0, G0 = gc.gravity_gradient(d0, q, GRAVITY, f)
    tau1, G1 = gc.gravity_gradient(d, to_q(q, pq, d.nq), GRAVITY, f)
    same(from_v(tau1, pv)[0], tau0, "tau")
    same(from_vv(G1, pv)[0], G0, "gradient")
    assert np.abs(keep_order(tau1, pv) - tau0).max() > 1.0e-3


@pytest.mark.parametrize("holes", [0, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_mass_matrix_inverse_checker_reads_the_maps(name, holes):
    d0, q, _ = states(name)
    d, pv, pq = scattered_maps(d0, np.random.default_rng(9), holes)
    full0 = mc.mass_matrix_inverse(OracleModel(d0), q)
    same(from_vv(mc.mass_matrix_inverse(OracleModel(d), to_q(q, pq, d.nq)), pv)[0], full0, "H^-1")
    cols = [3, 0, d0.nv - 1, 3]
    part = mc.mass_matrix_inverse(OracleModel(d), to_q(q, pq, d.nq), [int(pv[c]) for c in cols])
    same(part[:, pv, :], full0[:, :, cols], "listed columns")
    j = next(k for k in range(d0.n_joints) if int(d0.joint_type[k]) == 2)
    assert mc.joint_dofs(d, j) == [int(pv[r]) for r in mc.joint_dofs(d0, j)]


@pytest.mark.parametrize("name", list(MODELS))
def test_joint_limits_checker_reads_the_maps(name):
    """(without unowned indices: this checker inverts the oracle's H densely, and H has a zero row and column at an index no joint owns)"""
    d0, q, qd = states(name)
    d, pv, pq = scattered_maps(d0, np.random.default_rng(10))
    joints = jl.one_dof_joints(d0)[::-1][:6]  # (not ascending)
    _, c0 = jl.joint_indices(d0, joints)
    lower, upper = q[0, c0] - 0.05, q[0, c0] + 0.05  # row 0 sits inside; the other rows press on one side or the other
    r0 = jl.joint_limit_impulse(OracleModel(d0), d0, q, qd, joints, lower, upper, margin=0.01, erp=0.1, compliance=1.0e-6)
    r1 = jl.joint_limit_impulse(OracleModel(d), d, to_q(q, pq, d.nq), to_v(qd, pv, d.nv), joints, lower, upper, margin=0.01, erp=0.1, compliance=1.0e-6)
    assert r0["closed"].any() and np.array_equal(r0["closed"], r1["closed"])
    same(from_v(r1["qd_next"], pv)[0], r0["qd_next"], "qd_next")
    same(r1["impulse"], r0["impulse"], "impulse")
    same(r1["residual"], r0["residual"], "residual")
    assert np.array_equal(r1["d"], pv[r0["d"]]) and np.array_equal(r1["c"], pq[r0["c"]])
