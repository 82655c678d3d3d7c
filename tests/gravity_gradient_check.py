"""CPU checker of the gravity-gradient calls: an element-by-element restatement of MultiBodyGravityGradientCalculator
(algorithms/MultiBodyGravityGradientCalculator.java: passOne :397-481, passTwo :484-539, computeTauElement :541-563,
computeGravityGradientElement :565-588, computeSubTreeExtWrenchGradientElement :590-607, computeSingleExtWrenchGradientElement
:612-672) in numpy, one configuration at a time.  TEST INFRASTRUCTURE ONLY.

Frames and joint transforms are those of oracle/featherstone_np.py (link frames = Mecano's frames after the joints; its rotation,
quaternion and skew helpers are imported, not restated); the planar and spherical joints that module does not know are added here with
the conventions of include/mecano_hip.h.  Nothing of the device code's shortcuts is used: every entry is the reference's own sum of cross
and dot products, and the external-wrench part recurses over the descendants one wrench at a time as the reference does.
tests/test_gravity_gradient_cpu.py pins this file against the C oracle's inverse dynamics and a central finite difference of it.
"""
from __future__ import annotations

import numpy as np

from oracle import featherstone_np as fnp

REVOLUTE, PRISMATIC, SIXDOF, FIXED, PLANAR, SPHERICAL = 0, 1, 2, 3, 4, 5
NDOF = {REVOLUTE: 1, PRISMATIC: 1, SIXDOF: 6, FIXED: 0, PLANAR: 3, SPHERICAL: 3}
NCFG = {REVOLUTE: 1, PRISMATIC: 1, SIXDOF: 7, FIXED: 0, PLANAR: 3, SPHERICAL: 4}


class GravityModel:
    """The arrays of a ModelDesc the calculator reads, joints in desc order (parents first)."""

    def __init__(self, desc):
        n = self.n = int(desc.n_joints)
        self.nv, self.nq = int(desc.nv), int(desc.nq)
        self.parent = np.asarray(desc.parent, dtype=int)
        self.type = np.asarray(desc.joint_type, dtype=int)
        assert all(self.parent[i] < i for i in range(n)), "joints must be listed parents first"
        self.axis = np.asarray(desc.axis, dtype=float).reshape(n, 3)
        self.Xb = np.asarray(desc.X_before, dtype=float).reshape(n, 12)
        self.Xc = np.asarray(desc.X_com, dtype=float).reshape(n, 12)
        self.mass = np.asarray(desc.inertia_mass, dtype=float)
        self.com = np.asarray(desc.inertia_com, dtype=float).reshape(n, 3)
        ndof = np.array([NDOF[int(t)] for t in self.type], dtype=int)
        ncfg = np.array([NCFG[int(t)] for t in self.type], dtype=int)
        self.dof_ofs = np.concatenate([[0], np.cumsum(ndof)]).astype(int)
        self.cfg_ofs = np.concatenate([[0], np.cumsum(ncfg)]).astype(int)
        self.dof_idx = np.asarray(desc.dof_indices, dtype=int)
        self.cfg_idx = np.asarray(desc.cfg_indices, dtype=int)
        self.children = [[c for c in range(n) if self.parent[c] == i] for i in range(n)]

    def dofs(self, i):
        return self.dof_idx[self.dof_ofs[i]:self.dof_ofs[i + 1]]

    def unit_twists(self, i):
        """JointReadOnly.getUnitTwists(): (angular, linear) pairs in the frame after the joint, one per DoF."""
        t, z = int(self.type[i]), np.zeros(3)
        e = np.eye(3)
        if t == REVOLUTE:
            return [(self.axis[i], z)]
        if t == PRISMATIC:
            return [(z, self.axis[i])]
        if t == SIXDOF:
            return [(e[k], z) for k in range(3)] + [(z, e[k]) for k in range(3)]
        if t == PLANAR:  # w_y, v_x, v_z
            return [(e[1], z), (z, e[0]), (z, e[2])]
        if t == SPHERICAL:
            return [(e[k], z) for k in range(3)]
        return []

    def joint_pose(self, i, q):
        """(R, p) of the frame after joint i in the frame before it."""
        t = int(self.type[i])
        ci = self.cfg_idx[self.cfg_ofs[i]:self.cfg_ofs[i + 1]]
        if t == REVOLUTE:
            return fnp.rot_axis_angle(self.axis[i], q[ci[0]]), np.zeros(3)
        if t == PRISMATIC:
            return np.eye(3), q[ci[0]] * self.axis[i]
        if t == SIXDOF:
            return fnp.quat_to_R(q[ci[:4]]), q[ci[4:7]].copy()
        if t == SPHERICAL:
            return fnp.quat_to_R(q[ci[:4]]), np.zeros(3)
        if t == PLANAR:  # rotation about y by the pitch, translation (x, 0, z)
            return fnp.rot_axis_angle(np.array([0.0, 1.0, 0.0]), q[ci[0]]), np.array([q[ci[1]], 0.0, q[ci[2]]])
        return np.eye(3), np.zeros(3)

    def world_poses(self, q):
        """Poses in the root body frame of the frames after the joints and of the body-fixed frames: (Ra, pa, Rbody, pbody)."""
        Ra, pa, Rf, pf = [None] * self.n, [None] * self.n, [None] * self.n, [None] * self.n
        for i in range(self.n):
            p = self.parent[i]
            R0, p0 = (np.eye(3), np.zeros(3)) if p < 0 else (Ra[p], pa[p])
            Rb, pb = self.Xb[i, :9].reshape(3, 3), self.Xb[i, 9:]
            RJ, pJ = self.joint_pose(i, q)
            Ra[i] = R0 @ Rb @ RJ
            pa[i] = p0 + R0 @ (pb + Rb @ pJ)
            Rc, pc = self.Xc[i, :9].reshape(3, 3), self.Xc[i, 9:]
            Rf[i] = Ra[i] @ Rc
            pf[i] = pa[i] + Ra[i] @ pc
        return Ra, pa, Rf, pf


def gravity_gradient_one(m: GravityModel, q, gravity, f_ext=None):
    """(tau [nv], grad [nv, nv]) of one configuration.  f_ext: [n, 6] wrenches (moment, force) in the body-fixed frames, or None."""
    n = m.n
    g = np.asarray(gravity, dtype=float).reshape(3)
    Ra, pa, Rf, pf = m.world_poses(np.asarray(q, dtype=float))
    W = np.zeros((n, 6)) if f_ext is None else np.asarray(f_ext, dtype=float).reshape(n, 6)
    has_ext = [bool(np.any(W[i] != 0.0)) for i in range(n)]

    # ---- passOne, leaves to root: subtree mass, external spatial force, gravity force and centre of mass in the frames after the joints
    sub_mass = np.zeros(n)
    sub_ext = np.zeros((n, 6))  # (moment, force) about the origin of the frame after the joint
    sub_has = list(has_ext)
    sub_com = np.zeros((n, 3))
    g_force = np.zeros((n, 3))
    for i in range(n - 1, -1, -1):
        Rc, pc = m.Xc[i, :9].reshape(3, 3), m.Xc[i, 9:]
        sub_mass[i] = m.mass[i] + sum(sub_mass[c] for c in m.children[i])
        force = Rc @ W[i, 3:]
        sub_ext[i] = np.concatenate([Rc @ W[i, :3] + np.cross(pc, force), force])  # SpatialForce.changeFrame(frameAfterJoint)
        for c in m.children[i]:
            if sub_has[c]:
                R, p = Ra[i].T @ Ra[c], Ra[i].T @ (pa[c] - pa[i])
                force = R @ sub_ext[c, 3:]
                sub_ext[i] += np.concatenate([R @ sub_ext[c, :3] + np.cross(p, force), force])
                sub_has[i] = True
        g_force[i] = Ra[i].T @ (sub_mass[i] * g)
        com = m.mass[i] * (Rc @ m.com[i] + pc)
        for c in m.children[i]:
            com = com + sub_mass[c] * (Ra[i].T @ (pa[c] + Ra[c] @ sub_com[c] - pa[i]))
        sub_com[i] = com / sub_mass[i]

    def tau_element(i, w, v):
        f = -g_force[i]
        t = np.cross(sub_com[i], f) - sub_ext[i, :3]
        return float(np.dot(t, w) + np.dot(f - sub_ext[i, 3:], v))

    def gravity_element(k, twist_i, twist_j):
        (w_i, v_i), (w_j, _) = twist_i, twist_j
        f_dot = np.cross(-g_force[k], w_j)
        t_dot = np.cross(sub_com[k], f_dot)
        return float(np.dot(t_dot, w_i) + np.dot(f_dot, v_i))

    def single_ext_element(k, twist_i, twist_j, d):
        """The wrench of body d seen from the frame after joint k: only rotated, applied at the origin of d's body-fixed frame."""
        R = Ra[k].T @ Rf[d]
        f, t = -(R @ W[d, 3:]), -(R @ W[d, :3])
        dk = Ra[k].T @ (pf[d] - pa[k])
        (w_i, v_i), (w_j, v_j) = twist_i, twist_j
        f_dot_j, f_dot_i = np.cross(f, w_j), np.cross(f, w_i)
        t_dot_j = np.cross(dk, f_dot_j) + np.cross(t, w_j)
        t_dot_i = np.cross(dk, f_dot_i)
        return float(np.dot(t_dot_j, w_i) + np.dot(f_dot_j, v_i) - np.dot(t_dot_i, w_j) - np.dot(f_dot_i, v_j))

    def subtree_ext_element(k, twist_i, twist_j, start):
        if not sub_has[start]:
            return 0.0
        e = single_ext_element(k, twist_i, twist_j, start) if has_ext[start] else 0.0
        for c in m.children[start]:
            e += subtree_ext_element(k, twist_i, twist_j, c)
        return e

    # ---- passTwo
    tau = np.zeros(m.nv)
    grad = np.zeros((m.nv, m.nv))
    for k in range(n):
        idx, tw = m.dofs(k), m.unit_twists(k)
        for i in range(len(tw)):
            tau[idx[i]] = tau_element(k, *tw[i])
            grad[idx[i], idx[i]] = gravity_element(k, tw[i], tw[i])
            for j in range(i):
                e = subtree_ext_element(k, tw[i], tw[j], k)
                grad[idx[i], idx[j]] = gravity_element(k, tw[i], tw[j]) + e
                grad[idx[j], idx[i]] = gravity_element(k, tw[j], tw[i]) - e
        a = m.parent[k]
        while a >= 0:
            R, p = Ra[a].T @ Ra[k], Ra[a].T @ (pa[k] - pa[a])  # the frame after joint k in the frame after joint a
            ia = m.dofs(a)
            for j in range(len(tw)):
                for i, (w, v) in enumerate(m.unit_twists(a)):
                    twist_a = (R.T @ w, R.T @ (v + np.cross(w, p)))  # Twist.changeFrame(frameAfterJoint of k)
                    gv = gravity_element(k, tw[j], twist_a)
                    grad[ia[i], idx[j]] = gv
                    grad[idx[j], ia[i]] = gv + subtree_ext_element(k, tw[j], twist_a, k)
            a = m.parent[a]
    return tau, grad


def gravity_gradient(desc, q, gravity, f_ext=None):
    """Batched front end: q [B, nq], f_ext [B, n, 6] or None -> (tau [B, nv], grad [B, nv, nv])."""
    m = desc if isinstance(desc, GravityModel) else GravityModel(desc)
    q = np.asarray(q, dtype=float)
    B = q.shape[0]
    tau, grad = np.zeros((B, m.nv)), np.zeros((B, m.nv, m.nv))
    for b in range(B):
        tau[b], grad[b] = gravity_gradient_one(m, q[b], gravity, None if f_ext is None else np.asarray(f_ext)[b])
    return tau, grad


def related(desc):
    """[nv, nv] bool: True where the joints of the two DoFs are the same or one is an ancestor of the other."""
    m = desc if isinstance(desc, GravityModel) else GravityModel(desc)
    rel = np.zeros((m.nv, m.nv), dtype=bool)
    for k in range(m.n):
        a = k
        while a >= 0:
            rel[np.ix_(m.dofs(k), m.dofs(a))] = True
            rel[np.ix_(m.dofs(a), m.dofs(k))] = True
            a = m.parent[a]
    return rel


def wrenches_held_in_world(m: GravityModel, q0, q1, f_ext):
    """f_ext [n, 6] given in the body-fixed frames at q0, re-expressed in the body-fixed frames at q1 as the same spatial forces in
    the world (Wrench.changeFrame(worldFrame) before the step, setMatchingFrame after it)."""
    _, _, R0, p0 = m.world_poses(np.asarray(q0, dtype=float))
    _, _, R1, p1 = m.world_poses(np.asarray(q1, dtype=float))
    out = np.zeros((m.n, 6))
    for i in range(m.n):
        force_w = R0[i] @ f_ext[i, 3:]
        moment_w = R0[i] @ f_ext[i, :3] + np.cross(p0[i], force_w)
        out[i, 3:] = R1[i].T @ force_w
        out[i, :3] = R1[i].T @ (moment_w - np.cross(p1[i], force_w))
    return out
