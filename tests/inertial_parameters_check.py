"""CPU checker of mh_rnea_parameters_* / mh_aba_parameters_*: row r of a batch is evaluated by the C oracle on a model of its own,
``OracleModel(dataclasses.replace(desc, inertia_mass=..., inertia_com=..., inertia_J=...))`` built from row r's ten numbers per joint
(mass, com, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz in the description's joint order: OracleModel.parameter_vector), and a generator of physical
parameter sets around a description."""
import dataclasses

import numpy as np

from oracle.cpu_oracle import OracleModel

SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def parameters_of(desc):
    """[n_joints, 10] of a description: what mh_model_inertial_parameters returns (the symmetric part of J)."""
    n = desc.n_joints
    J = np.asarray(desc.inertia_J, dtype=np.float64).reshape(n, 3, 3)
    pi = np.zeros((n, 10))
    pi[:, 0] = np.asarray(desc.inertia_mass, dtype=np.float64)
    pi[:, 1:4] = np.asarray(desc.inertia_com, dtype=np.float64).reshape(n, 3)
    for c, (a, b) in enumerate(SYM):
        pi[:, 4 + c] = 0.5 * (J[:, a, b] + J[:, b, a])
    return pi


def desc_with(desc, pi):
    """The description with the inertia of every body replaced by pi [n_joints, 10]."""
    n = desc.n_joints
    pi = np.asarray(pi, dtype=np.float64).reshape(n, 10)
    J = np.zeros((n, 3, 3))
    for c, (a, b) in enumerate(SYM):
        J[:, a, b] = J[:, b, a] = pi[:, 4 + c]
    return dataclasses.replace(desc, inertia_mass=pi[:, 0].copy(), inertia_com=pi[:, 1:4].reshape(-1).copy(), inertia_J=J.reshape(-1))


class Checker:
    """rnea / aba / crba of a batch whose row r has its own parameters pi[r]; one OracleModel per distinct parameter set (cached)."""

    def __init__(self, desc):
        self.desc = desc
        self._models = {}
        self._own = parameters_of(desc)

    def model(self, pi_row):
        pi_row = np.ascontiguousarray(pi_row, dtype=np.float64).reshape(self.desc.n_joints, 10)
        key = pi_row.tobytes()
        if key not in self._models:
            # the description's own numbers replace nothing: the description as it is (a lumped body's J is symmetric only up to rounding,
            # and ten numbers cannot carry its skew part)
            self._models[key] = OracleModel(self.desc if np.array_equal(pi_row, self._own) else desc_with(self.desc, pi_row))
        return self._models[key]

    def _rows(self, fn, pi, n_out):
        pi = np.asarray(pi, dtype=np.float64).reshape(len(pi), -1)
        out = np.zeros((pi.shape[0], n_out))
        for r in range(pi.shape[0]):
            out[r] = fn(self.model(pi[r]), r)
        return out

    def rnea(self, q, qd, qdd, pi, gravity=(0.0, 0.0, -9.81), f_ext=None, consider_coriolis=True, consider_accelerations=True):
        """consider_coriolis=False is evaluated as qd = 0 with the switch ON.  With the switch off, a body whose centre of mass is off the
        origin of its body-fixed frame -- every body of a generated parameter set -- takes the oracle down Mecano's offset-CoM branch
        without a twist, which leaves the moment c x a unscaled by the mass (oracle/mecano_oracle.c: dynamic_wrench,
        MecanoTools.java:650-692); qd = 0 gives the same efforts through the branch that scales, which is what mh_rnea_* computes
        (tests/test_gravity_gradient_cpu.py: holding_efforts does the same).  With every c = 0 the two are the same bits
        (tests/test_inertial_parameters_cpu.py pins that)."""
        if not consider_coriolis:
            qd, consider_coriolis = np.zeros_like(qd), True
        f = lambda r: None if f_ext is None else np.asarray(f_ext)[r:r + 1]
        return self._rows(lambda om, r: om.rnea(q[r:r + 1], qd[r:r + 1], qdd[r:r + 1], gravity, f(r), consider_coriolis, consider_accelerations)[0],
                          pi, self.desc.nv)

    def aba(self, q, qd, tau, pi, gravity=(0.0, 0.0, -9.81), f_ext=None):
        f = lambda r: None if f_ext is None else np.asarray(f_ext)[r:r + 1]
        return self._rows(lambda om, r: om.aba(q[r:r + 1], qd[r:r + 1], tau[r:r + 1], gravity, f(r))[0], pi, self.desc.nv)

    def crba(self, q, pi):
        """H of every row with its own parameters, [B, nv, nv]: cond_inf(H) of helpers.close_aba's per-row bound."""
        pi = np.asarray(pi, dtype=np.float64).reshape(len(pi), -1)
        return np.stack([self.model(pi[r]).crba(q[r:r + 1])[0] for r in range(pi.shape[0])])


def first_moment_form(pi):
    """(m, m c, J) of (m, c, J): the parameters the inverse dynamics is linear in (regressor with first_moment_columns)."""
    out = np.array(pi, dtype=np.float64).reshape(-1, 10).copy()
    out[:, 1:4] *= out[:, 0:1]
    return out.reshape(np.shape(pi))


def first_moment_regressor(desc, q, qd, qdd, gravity):
    """OracleModel.regressor with d tau / d (m c) in columns 1..3 of every body instead of the reference's zeros: a unit mass at a
    unit offset has (m, m c, J) = (1, e_k, 0), so the column is that model's inverse dynamics minus the mass column."""
    om = OracleModel(desc)
    Y = om.regressor(q, qd, qdd, gravity)
    n = desc.n_joints
    for i in range(n):
        for k in range(3):
            pi = np.zeros((n, 10))
            pi[i, 0], pi[i, 1 + k] = 1.0, 1.0
            Y[:, :, 10 * i + 1 + k] = OracleModel(desc_with(desc, pi)).rnea(q, qd, qdd, gravity) - Y[:, :, 10 * i]
    return Y


def _rotation(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def physical_parameter_sets(desc, rng, count):
    """[count, n_joints, 10]: physical inertias around the description's.  Per body: mass x U(0.5, 2); the central inertia x one
    U(0.5, 2) factor, turned by a random rotation of at most 0.3 rad; the centre of mass moved by U(-0.05, 0.05) per axis; J shifted
    back to the origin of the body-fixed frame (J = Jc + m (|c|^2 1 - c c^T))."""
    base = parameters_of(desc)
    n = desc.n_joints
    out = np.zeros((count, n, 10))
    for s in range(count):
        for i in range(n):
            m, c = base[i, 0], base[i, 1:4]
            J = np.zeros((3, 3))
            for k, (a, b) in enumerate(SYM):
                J[a, b] = J[b, a] = base[i, 4 + k]
            Jc = J - m * (c @ c * np.eye(3) - np.outer(c, c))
            R = _rotation(rng, 0.3)
            m2 = m * rng.uniform(0.5, 2.0)
            Jc2 = rng.uniform(0.5, 2.0) * (R @ Jc @ R.T)
            c2 = c + rng.uniform(-0.05, 0.05, 3)
            J2 = Jc2 + m2 * (c2 @ c2 * np.eye(3) - np.outer(c2, c2))
            J2 = 0.5 * (J2 + J2.T)
            out[s, i, 0], out[s, i, 1:4] = m2, c2
            out[s, i, 4:] = [J2[a, b] for a, b in SYM]
    return out
