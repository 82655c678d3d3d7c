"""CPU checker of mh_body_poses_* and mh_geometric_jacobian_*: poses, geometric Jacobians and convective terms from composed 4 x 4
transforms and unit twists, one configuration at a time (numpy; small cases only).

Frames and joint transforms are those of oracle/featherstone_np.py (link frames = Mecano's frames after the joints): KinModel is its
Model with the planar and spherical joints added, and everything below is built on its `X_child_to_parent` and `S`.  The chain between
base and end effector is collected by climbing the parents, as MultiBodySystemTools.collectJointPath does (tools/MultiBodySystemTools.java:
170-207); the Jacobian follows GeometricJacobianCalculator.updateJacobianMatrix (algorithms/GeometricJacobianCalculator.java:249-279) and the
convective term its updateJacobianRateMatrix / computeJacobianRateMatrixBlock (:316-377) step by step.  The dense body Jacobians of
featherstone_np (`_body_jacobians`) are not used here: tests/test_kinematics_cpu.py holds this file against them, and against facts that
come from the C oracle's dynamics."""
import math

import numpy as np

from oracle import featherstone_np as fnp

REVOLUTE, PRISMATIC, SIXDOF, FIXED, PLANAR, SPHERICAL = 0, 1, 2, 3, 4, 5
NDOF = {REVOLUTE: 1, PRISMATIC: 1, SIXDOF: 6, FIXED: 0, PLANAR: 3, SPHERICAL: 3}
NCFG = {REVOLUTE: 1, PRISMATIC: 1, SIXDOF: 7, FIXED: 0, PLANAR: 3, SPHERICAL: 4}
IDENTITY12 = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


class KinModel(fnp.Model):
    """featherstone_np.Model for every joint kind of a ModelDesc: the kinematic arrays only (no inertias)."""

    def __init__(self, desc):
        n = self.n = int(desc.n_joints)
        self.d = desc
        self.parent = np.asarray(desc.parent, dtype=int)
        self.type = np.asarray(desc.joint_type, dtype=int)
        assert all(self.parent[i] < i for i in range(n)), "joints must be listed parents first"
        self.axis = np.asarray(desc.axis, dtype=float).reshape(n, 3)
        self.Xb = np.asarray(desc.X_before, dtype=float).reshape(n, 12)
        self.Xc = np.asarray(desc.X_com, dtype=float).reshape(n, 12)
        self.ndof = np.array([NDOF[int(t)] for t in self.type], dtype=int)
        self.ncfg = np.array([NCFG[int(t)] for t in self.type], dtype=int)
        self.dof_ofs = np.concatenate([[0], np.cumsum(self.ndof)]).astype(int)
        self.cfg_ofs = np.concatenate([[0], np.cumsum(self.ncfg)]).astype(int)
        self.dof_idx = np.asarray(desc.dof_indices, dtype=int)
        self.cfg_idx = np.asarray(desc.cfg_indices, dtype=int)
        self.nv, self.nq = int(desc.nv), int(desc.nq)

    def cfgs(self, i):
        return self.cfg_idx[self.cfg_ofs[i]:self.cfg_ofs[i + 1]]

    def S(self, i):
        t = int(self.type[i])
        if t == PLANAR:  # w_y, v_x, v_z in the frame after the joint (PlanarJointReadOnly)
            S = np.zeros((6, 3))
            S[1, 0] = S[3, 1] = S[5, 2] = 1.0
            return S
        if t == SPHERICAL:
            return np.eye(6)[:, :3]
        return super().S(i)

    def X_child_to_parent(self, i, q):
        t = int(self.type[i])
        if t not in (PLANAR, SPHERICAL):
            return super().X_child_to_parent(i, q)
        ci = self.cfgs(i)
        Rb, pb = self.Xb[i, :9].reshape(3, 3), self.Xb[i, 9:]
        if t == SPHERICAL:
            RJ, pJ = fnp.quat_to_R(q[ci[:4]]), np.zeros(3)
        else:  # rotation about y by the pitch, translation (x, 0, z)
            RJ, pJ = fnp.rot_axis_angle(np.array([0.0, 1.0, 0.0]), q[ci[0]]), np.array([q[ci[1]], 0.0, q[ci[2]]])
        return fnp.plucker_motion(Rb, pb) @ fnp.plucker_motion(RJ, pJ)


# ---- 4 x 4 transforms <-> 6 x 6 motion transforms <-> 12 numbers
def T_of(R, p):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, p
    return T


def T_of12(pose):
    pose = np.asarray(pose, dtype=float).reshape(12)
    return T_of(pose[:9].reshape(3, 3), pose[9:])


def T_to12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def T_of_plucker(X):
    """The pose (child in parent) behind a motion transform child -> parent, X = [[R, 0], [skew(p) R, R]]."""
    R = X[:3, :3]
    P = X[3:, :3] @ R.T
    return T_of(R, np.array([P[2, 1], P[0, 2], P[1, 0]]))


def Ad(T):
    """Motion transform child -> parent of a pose (child in parent)."""
    return fnp.plucker_motion(T[:3, :3], T[:3, 3])


def T_inv(T):
    return T_of(T[:3, :3].T, -T[:3, :3].T @ T[:3, 3])


def joint_frames(m: KinModel, q):
    """Pose in the root body frame of the frame after every joint: composed 4 x 4 transforms."""
    T0 = [None] * m.n
    for i in range(m.n):
        T = T_of_plucker(m.X_child_to_parent(i, q))
        T0[i] = T if m.parent[i] < 0 else T0[m.parent[i]] @ T
    return T0


def frame_of(m: KinModel, T0, joint, pose=None):
    """Pose in the root body frame of a frame fixed in the successor body of `joint` (-1: the root body) at `pose` relative to the
    body-fixed frame."""
    T = np.eye(4) if joint < 0 else T0[joint] @ T_of12(m.Xc[joint])
    return T if pose is None else T @ T_of12(pose)


def joint_chain(m: KinModel, base, target):
    """[(joint, sign)] from the base to the end effector: the joints climbed from the base to the common ancestor enter inverted."""
    def ancestors(j):
        out = []
        while j >= 0:
            out.append(j)
            j = int(m.parent[j])
        return out
    up, down = ancestors(int(base)), ancestors(int(target))
    while up and down and up[-1] == down[-1]:  # what both climbs share lies above the common ancestor
        up.pop(), down.pop()
    return [(j, -1.0) for j in up] + [(j, 1.0) for j in reversed(down)]


def body_poses(m: KinModel, q, targets=None, poses=None):
    """[B, K, 12]: what mh_body_poses_* returns in AoS."""
    q = np.asarray(q, dtype=float)
    targets = list(range(m.n)) if targets is None else [int(t) for t in targets]
    K = len(targets)
    poses = np.tile(IDENTITY12, (K, 1)) if poses is None else np.asarray(poses, dtype=float).reshape(K, 12)
    out = np.zeros((q.shape[0], K, 12))
    for r in range(q.shape[0]):
        T0 = joint_frames(m, q[r])
        for k, t in enumerate(targets):
            out[r, k] = T_to12(frame_of(m, T0, t, poses[k]))
    return out


def compact_jacobian(m: KinModel, T0, base, target, pose=None):
    """(chain, J [6, chain DoFs]) in the reference's layout: columns in base-to-end-effector joint order, expressed in the target frame."""
    chain = joint_chain(m, base, target)
    to_target = Ad(T_inv(frame_of(m, T0, target, pose)))
    cols = [sign * (to_target @ Ad(T0[j]) @ m.S(j)) for j, sign in chain]
    return chain, (np.concatenate(cols, axis=1) if cols else np.zeros((6, 0)))


def convective_term(m: KinModel, chain, Jc, qd):
    """updateJacobianRateMatrix (:316-349): the columns of the last joint get zeros, every joint before it
    J_col x (twist of the end effector relative to what follows the joint), then Jdot qd."""
    if not chain:
        return np.zeros(6)
    nd = [int(m.ndof[j]) for j, _ in chain]
    qc = np.concatenate([np.asarray(qd, dtype=float)[m.dofs(j)] for j, _ in chain]) if sum(nd) else np.zeros(0)
    Jd = np.zeros_like(Jc)
    end = Jc.shape[1]
    start = end - nd[-1]
    twist = np.zeros(6)
    for idx in range(len(chain) - 2, -1, -1):
        twist = twist + Jc[:, start:end] @ qc[start:end]  # addJointTwist
        end = start
        start -= nd[idx]
        for c in range(start, end):  # computeJacobianRateMatrixBlock (:362-377)
            w, v = Jc[:3, c], Jc[3:, c]
            Jd[3:, c] = np.cross(v, twist[:3]) + np.cross(w, twist[3:])
            Jd[:3, c] = np.cross(w, twist[:3])
    return Jd @ qc


def geometric_jacobian(m: KinModel, q, targets, bases=None, poses=None, qd=None):
    """(J [B, 6 K, nv], c [B, K, 6] or None): what mh_geometric_jacobian_* returns in AoS."""
    q = np.asarray(q, dtype=float)
    targets = [int(t) for t in targets]
    K = len(targets)
    bases = [-1] * K if bases is None else [int(b) for b in bases]
    poses = np.tile(IDENTITY12, (K, 1)) if poses is None else np.asarray(poses, dtype=float).reshape(K, 12)
    B = q.shape[0]
    J = np.zeros((B, 6 * K, m.nv))
    c = None if qd is None else np.zeros((B, K, 6))
    for r in range(B):
        T0 = joint_frames(m, q[r])
        for k in range(K):
            chain, Jc = compact_jacobian(m, T0, bases[k], targets[k], poses[k])
            col = 0
            for j, _ in chain:
                for d in m.dofs(j):
                    J[r, 6 * k:6 * k + 6, d] = Jc[:, col]
                    col += 1
            if qd is not None:
                c[r, k] = convective_term(m, chain, Jc, np.asarray(qd, dtype=float)[r])
    return J, c


# ---- q (+) dq: the step MultiBodySystemStateIntegrator applies (a twist increment in the frame after a floating / planar / spherical joint)
def _quat_mul(a, b):
    ax, ay, az, as_ = a
    bx, by, bz, bs = b
    return np.array([as_ * bx + ax * bs + ay * bz - az * by, as_ * by - ax * bz + ay * bs + az * bx, as_ * bz + ax * by - ay * bx + az * bs,
                     as_ * bs - ax * bx - ay * by - az * bz])


def _quat_exp(r):
    th = float(np.linalg.norm(r))
    if th < 1.0e-12:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([math.sin(0.5 * th) / th * np.asarray(r), [math.cos(0.5 * th)]])


def configuration_add(m: KinModel, q, dq):
    q = np.asarray(q, dtype=float)
    out = q.copy()
    for i in range(m.n):
        t, ci, di = int(m.type[i]), m.cfgs(i), m.dofs(i)
        if t in (REVOLUTE, PRISMATIC):
            out[ci[0]] = q[ci[0]] + dq[di[0]]
        elif t == PLANAR:
            c, s = math.cos(q[ci[0]]), math.sin(q[ci[0]])
            out[ci[0]] = q[ci[0]] + dq[di[0]]
            out[ci[1]] = q[ci[1]] + c * dq[di[1]] + s * dq[di[2]]
            out[ci[2]] = q[ci[2]] - s * dq[di[1]] + c * dq[di[2]]
        elif t in (SPHERICAL, SIXDOF):
            out[ci[:4]] = _quat_mul(q[ci[:4]], _quat_exp(dq[di[:3]]))
            if t == SIXDOF:
                out[ci[4:7]] = q[ci[4:7]] + fnp.quat_to_R(q[ci[:4]]) @ dq[di[3:6]]
    return out


def twist_of_difference(T_minus, T_plus, T, eps):
    """Body twist (angular, linear) of a frame from its poses at q (-) eps e and q (+) eps e: T^-1 (T+ - T-) / (2 eps)."""
    D = T_inv(T) @ (T_plus - T_minus) / (2.0 * eps)
    return np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1], 2 * D[0, 3], 2 * D[1, 3], 2 * D[2, 3]]) / 2.0


def random_poses(rng, K):
    """K poses: a random rotation and an offset of up to 0.3 m each"""
    from mecano_amd import random_tools as rt
    out = np.zeros((K, 12))
    for k in range(K):
        out[k, :9] = rt.quaternionToMatrix(rt.nextQuaternion(rng)).reshape(9)
        out[k, 9:] = rng.uniform(-0.3, 0.3, 3)
    return out


def motion_into_frame(pose):
    """6 x 6: a motion vector in the body-fixed frame -> in a frame at `pose` relative to it."""
    return Ad(T_inv(T_of12(pose)))
