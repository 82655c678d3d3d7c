"""A closed kinematic loop on the device: 1024 parallelogram linkages, each with its loop closed by a constraint between two moving bodies.

    python examples/closed_loop_four_bar.py [steps]

Two cranks of length L = 0.6 m turn about z on the ground, d = 0.9 m apart; the coupler hangs on the tip of crank A.  The tree has three
revolute joints (crank A, coupler, crank D); the fourth hinge, between the far end of the coupler and the tip of crank D, is no joint of the
tree: it is held by mh_aba_constrained_between_f64 -- target the coupler at its far end, base crank D, the two linear rows in the plane.
The linkages start at random crank angles with the loop closed, at rest, and swing under gravity with a little damping at the cranks.
Every step solves the constrained forward dynamics (HipModel.aba_constrained(..., bases=...)) and integrates (mh_integrate_f64).  The
constraint is on accelerations, so the integrator's position error would accumulate: a_des carries the Baumgarte terms
-2 w (J qd) - w^2 (gap), with J from mh_geometric_jacobian_f64 for the same base and the gap from mh_body_poses_f64.  Nothing inside the
loop reads a value back to the host.

It prints the loop-closure error (the distance between the two halves of the fourth hinge) after the run, with and without the Baumgarte
terms, beside the coupler's tilt (a parallelogram keeps q_coupler = -q_crank_a), and checks that the terms reduce the error.
Needs a built library (python -m mecano_amd.build) and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd.engine import HipModel
from mecano_amd.multibody import MultiBodySystem, RevoluteJoint, RigidBody

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
B, dt = 1024, 1.0e-3
L, D = 0.6, 0.9
OMEGA = 100.0        # 1 / s: critically damped error dynamics, well inside 2 / dt
CRANK_DAMPING = 0.2  # N m s / rad
GRAVITY = (0.0, -9.81, 0.0)
Z = (0.0, 0.0, 1.0)


def pose(x):
    return np.concatenate([np.eye(3).reshape(9), [x, 0.0, 0.0]])


ground = RigidBody("ground")
joint_a = RevoluteJoint("crank_a", ground, None, Z)
crank_a = RigidBody("a", joint_a, np.diag([0.01, 0.01, 0.05]), 1.3, inertiaPose=pose(0.25))
joint_c = RevoluteJoint("coupler", crank_a, (np.eye(3), np.array([L, 0.0, 0.0])), Z)
RigidBody("c", joint_c, np.diag([0.01, 0.01, 0.07]), 0.8, inertiaPose=pose(D / 2))
joint_d = RevoluteJoint("crank_d", ground, (np.eye(3), np.array([D, 0.0, 0.0])), Z)
RigidBody("d", joint_d, np.diag([0.01, 0.01, 0.05]), 1.3, inertiaPose=pose(0.25))
model = HipModel(MultiBodySystem.toMultiBodySystemInput(ground).toModelDesc())

COUPLER, CRANK_D = 1, 2
TARGETS, BASES, ROWS = [COUPLER], [CRANK_D], [0b011000]  # linear x and y of the hinge frame on the coupler
HINGE = pose(D / 2)[None]                                # from the coupler's centre-of-mass frame to its far end
HALVES = np.stack([pose(D / 2), pose(L - 0.25)])         # the same point on the coupler and on crank D, each from its body-fixed frame


def run(stabilised):
    """(loop-closure error in metres after the run, worst |q_coupler + q_crank_a|)"""
    theta = torch.tensor(np.random.default_rng(0).uniform(-np.pi, np.pi, B), device="cuda")
    q = torch.stack([theta, -theta, theta], dim=1).contiguous()
    qd = torch.zeros_like(q)
    a_des = torch.zeros((B, 1, 6), dtype=torch.float64, device="cuda")
    qdd, lam = torch.empty_like(qd), torch.empty_like(a_des)
    J, halves = torch.empty((B, 6, 3), dtype=torch.float64, device="cuda"), torch.empty((B, 2, 12), dtype=torch.float64, device="cuda")
    for _ in range(steps):
        if stabilised:
            model.geometric_jacobian(q, TARGETS, BASES, HINGE, out=J)
            model.body_poses(q, [COUPLER, CRANK_D], HALVES, out=halves)
            R = halves[:, 0, :9].reshape(B, 3, 3)
            gap = torch.einsum("bji,bj->bi", R, halves[:, 0, 9:] - halves[:, 1, 9:])  # in the hinge frame of the coupler
            a_des[:, 0, 3:] = -2.0 * OMEGA * torch.einsum("bij,bj->bi", J[:, 3:], qd) - OMEGA * OMEGA * gap
        tau = torch.zeros_like(qd)
        tau[:, 0], tau[:, 2] = -CRANK_DAMPING * qd[:, 0], -CRANK_DAMPING * qd[:, 2]
        model.aba_constrained(q, qd, tau, TARGETS, ROWS, HINGE, a_des=a_des, gravity=GRAVITY, out=(qdd, lam), bases=BASES)
        model.integrate(dt, q, qd, qdd, out=(q, qd))
    halves = model.body_poses(q, [COUPLER, CRANK_D], HALVES)
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(qd).all(), "the state blew up"
    return float((halves[:, 0, 9:] - halves[:, 1, 9:]).norm(dim=1).max()), float((q[:, 0] + q[:, 1]).abs().max())


gap_s, skew_s = run(True)
gap_p, skew_p = run(False)
print(f"{steps} steps of {dt * 1e3:.0f} ms, {B} parallelogram linkages: loop-closure error {gap_s * 1e3:.2e} mm with the Baumgarte terms "
      f"(coupler tilt {skew_s:.1e} rad), {gap_p * 1e3:.2e} mm without ({skew_p:.1e} rad)")
assert gap_s < gap_p, "the Baumgarte terms did not reduce the loop-closure error"
print("self-check passed")
