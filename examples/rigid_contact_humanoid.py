"""Rigid contact without leaving the device: 4096 limp 30-DoF humanoids with both feet welded to where they start.

    python examples/rigid_contact_humanoid.py [steps]

The robots start in random attitudes with random joint velocities.  mh_constraint_impulse_f64 first stops the feet (the velocity-level
solve of a touch-down); then every step computes the acceleration that keeps both foot frames where they are (mh_aba_constrained_f64, a
weld per foot: 12 rows) and integrates it (mh_integrate_f64).  The constraint is on accelerations, so position errors of the integrator
would accumulate: the desired acceleration carries the usual stabilising terms a_des = -2 w (J qd) - w^2 (pose error), formed on the device
from mh_body_poses_f64 and mh_geometric_jacobian_f64.  Nothing inside the loop reads a value back to the host.  Against the penalty
ground of examples/ground_contact_humanoid.py there is no stiffness to choose, no sinking, and the step is five times longer.

It ends with a self-check that is relational, not a tuned number: at every step the constraint equation J_c qdd + c = a_des holds on the
device outputs to the bound the tests hold it to -- 8 sqrt(8 n) cond_inf(H) u times the magnitude of its terms, J and c from
mh_geometric_jacobian_f64 and H from mh_crba_f64 --, and the feet end closer to where they started than in the same run without the
stabilising terms.  Needs a built library (python -m mecano_amd.build) and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
B, dt, g = 4096, 5.0e-3, 9.81
FEET, WELD = [6, 12], [0b111111, 0b111111]  # last joints of the two leg chains; all six rows of each foot frame
OMEGA = 40.0                                # 1 / s: critically damped error dynamics, well inside 2 / dt
JOINT_DAMPING = 0.5                         # N m s / rad

system = rt.nextHumanoid(np.random.default_rng(43))
desc = system.toModelDesc()
model = HipModel(desc)
model.reserve(B)
n, nv = desc.n_joints, desc.nv
joint_damping = torch.full((nv,), JOINT_DAMPING, dtype=torch.float64, device="cuda")
joint_damping[[int(i) for i in desc.dof_indices[:6]]] = 0.0  # the floating base is free
factor, u = 8.0 * (8.0 * n) ** 0.5, 2.0 ** -53


def run(stabilised):
    """(worst residual of the constraint equation over its bound, over all steps and robots; final drift of the feet in metres)"""
    q, qd, _, _ = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(0), system, B))
    start = model.body_poses(q, FEET)  # [B, 2, 12]: R row-major, p
    R0, p0 = start[:, :, :9].reshape(B, 2, 3, 3), start[:, :, 9:]
    qd, _ = model.constraint_impulse(q, qd, FEET, WELD)  # touch-down: both feet stop
    pose = torch.empty_like(start)
    J, c = torch.empty((B, 12, nv), dtype=torch.float64, device="cuda"), torch.empty((B, 2, 6), dtype=torch.float64, device="cuda")
    a_des = torch.zeros((B, 2, 6), dtype=torch.float64, device="cuda")
    qdd, lam = torch.empty_like(qd), torch.empty_like(a_des)
    worst = torch.zeros((), dtype=torch.float64, device="cuda")
    for _ in range(steps):
        model.geometric_jacobian(q, FEET, qd=qd, convective=True, out=(J, c))
        if stabilised:
            model.body_poses(q, FEET, out=pose)
            R, p = pose[:, :, :9].reshape(B, 2, 3, 3), pose[:, :, 9:]
            E = torch.einsum("bkji,bkjl->bkil", R0, R)  # R0^T R: the rotation since the start, in the foot's frame to first order
            e_rot = 0.5 * torch.stack([E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]], dim=-1)
            e_pos = torch.einsum("bkji,bkj->bki", R, p - p0)
            twist = torch.einsum("bij,bj->bi", J, qd).view(B, 2, 6)
            a_des = -2.0 * OMEGA * twist - OMEGA * OMEGA * torch.cat([e_rot, e_pos], dim=-1)
        model.aba_constrained(q, qd, -joint_damping * qd, FEET, WELD, a_des=a_des, gravity=(0.0, 0.0, -g), out=(qdd, lam))
        residual = (torch.einsum("bij,bj->bi", J, qdd) + c.view(B, 12) - a_des.view(B, 12)).abs().amax(dim=1)
        scale = (torch.einsum("bij,bj->bi", J.abs(), qdd.abs()) + c.view(B, 12).abs() + a_des.view(B, 12).abs()).amax(dim=1).clamp(min=1.0)
        cond = torch.linalg.cond(model.crba(q), p=float("inf"))
        worst = torch.maximum(worst, (residual / (factor * cond * u * scale)).max())
        model.integrate(dt, q, qd, qdd, out=(q, qd))
    end = model.body_poses(q, FEET)
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(qd).all(), "the state blew up"
    return float(worst), float((end[:, :, 9:] - p0).norm(dim=2).max())


ratio_s, drift_s = run(True)
ratio_p, drift_p = run(False)
print(f"{steps} steps of {dt * 1e3:.0f} ms, {B} humanoids, both feet welded: constraint residual / bound {ratio_s:.3f} with the stabilising terms, "
      f"{ratio_p:.3f} without; the feet end {drift_s * 1e3:.3f} mm from their start with them, {drift_p * 1e3:.3f} mm without")
assert ratio_s <= 1.0 and ratio_p <= 1.0, "the constraint equation does not hold to its bound"
assert drift_s < drift_p, "the stabilising terms did not reduce the drift of the feet"
print("self-check passed")
