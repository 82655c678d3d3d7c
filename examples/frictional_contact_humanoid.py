"""Frictional ground contact without leaving the device: 4096 limp 30-DoF humanoids dropped on a plane, four contact points under each foot.

    python examples/frictional_contact_humanoid.py [steps]

A velocity-level time-stepping scheme.  Every step finds, on the device, which of the eight sole corners are at or below the ground
(mh_body_poses_f64), the free acceleration (mh_aba_f64) and with it the velocity the robots would have without the ground, and hands that
to mh_contact_impulse_f64: the corners that are closed press, stick or slide inside their friction cones, the others carry nothing.  The
least normal velocity asked of a closed corner removes a share BETA of its depth per step (Baumgarte), the impulses of the step before
start the sweeps (the output is its own warm start), and mh_configuration_add_f64 moves the configuration by dt qd+.  Nothing inside the
loop reads a value back to the host.  Four corners of one rigid sole are twelve rows of rank six: the compliance carries the solve.

It ends with a relational self-check: no closed contact ever carried a negative normal impulse, every impulse lay inside its friction
cone to rounding, and the deepest any corner sank is less than the deepest foot of examples/ground_contact_humanoid.py -- the penalty
ground, run here for the same number of steps.
Needs a built library (python -m mecano_amd.build) and an MI355X."""
import os
import runpy
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
B, dt, g = 4096, 1.0e-3, 9.81
MU, BETA, COMPLIANCE, SWEEPS = 0.7, 0.2, 1.0e-4, 50
JOINT_DAMPING = 0.5  # N m s/rad, as in the penalty example
FEET = [6, 12]       # last joints of the two leg chains
TARGETS = [FEET[0]] * 4 + [FEET[1]] * 4
K = len(TARGETS)
CORNERS = np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (K, 1))
for k in range(K):  # a 0.2 m x 0.1 m sole around the body-fixed frame of the foot
    CORNERS[k, 9:] = (0.1 if k & 1 else -0.1, 0.05 if k & 2 else -0.05, 0.0)

system = rt.nextHumanoid(np.random.default_rng(43))
desc = system.toModelDesc()
model = HipModel(desc)
model.reserve(B)

q, qd, _, _ = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(0), system, B))
qd.zero_()
pelvis_z = int(desc.cfg_indices[6])  # the floating joint's configuration is (qx, qy, qz, qs, x, y, z)
# every robot starts with its lowest corner 2 cm above the ground (z = 0)
q[:, pelvis_z] += 0.02 - model.body_poses(q, TARGETS, CORNERS)[:, :, 11].amin(dim=1)

joint_damping = torch.full((desc.nv,), JOINT_DAMPING, dtype=torch.float64, device="cuda")
joint_damping[[int(i) for i in desc.dof_indices[:6]]] = 0.0  # the floating base is free
corner = torch.empty((B, K, 12), dtype=torch.float64, device="cuda")
qd_next = torch.empty_like(qd)
impulse = torch.zeros((B, K, 6), dtype=torch.float64, device="cuda")
residual = torch.empty(B, dtype=torch.float64, device="cuda")
mu = [MU] * K

lowest = torch.full((), float("inf"), dtype=torch.float64, device="cuda")
least_normal = torch.full((), float("inf"), dtype=torch.float64, device="cuda")   # smallest normal impulse of a closed contact
worst_cone = torch.full((), -float("inf"), dtype=torch.float64, device="cuda")   # largest |tangential| - mu normal
largest = torch.zeros((), dtype=torch.float64, device="cuda")
touched = torch.zeros(B, dtype=torch.bool, device="cuda")
for _ in range(steps):
    model.body_poses(q, TARGETS, CORNERS, out=corner)
    height = corner[:, :, 11]
    active = (height <= 0.0).to(torch.int32)
    v_normal = (-BETA / dt * height).contiguous()
    qdd = model.aba(q, qd, -joint_damping * qd, (0.0, 0.0, -g))
    v_free = qd + dt * qdd
    model.contact_impulse(q, v_free, TARGETS, mu, CORNERS, None, active, v_normal, COMPLIANCE, SWEEPS, init=impulse, out=(qd_next, impulse, residual))
    qd, qd_next = qd_next, qd
    model.configuration_add(q, dt * qd, out=q)
    # the record of the self-check, kept on the device: the normal in the target frame is R^T e_z, the third row of R
    lam = impulse[:, :, 3:]
    normal = (corner[:, :, 6:9] * lam).sum(dim=2)
    tangential = (lam - normal[:, :, None] * corner[:, :, 6:9]).norm(dim=2)
    lowest = torch.minimum(lowest, height.amin())
    least_normal = torch.minimum(least_normal, normal.amin())
    worst_cone = torch.maximum(worst_cone, (tangential - MU * normal).amax())
    largest = torch.maximum(largest, lam.abs().amax())
    touched |= active.any(dim=1)
torch.cuda.synchronize()

lowest, least_normal, worst_cone, largest, landed = float(lowest), float(least_normal), float(worst_cone), float(largest), int(touched.sum())
print(f"{steps} steps of {B} humanoids: {landed} touched the ground, deepest corner {-lowest * 1e3:.2f} mm below it, largest impulse {largest:.3f} N s, "
      f"least normal impulse {least_normal:.2e}, worst |tangential| - mu normal {worst_cone:.2e}, last residual <= {float(residual.max()):.2e}")
assert torch.isfinite(q).all() and torch.isfinite(qd).all(), "the state blew up"
assert landed == B or steps < 200, "some robot never reached the ground"
rounding = 1.0e-12 * max(1.0, largest)
assert least_normal >= -rounding, f"a closed contact pulled: normal impulse {least_normal}"
assert worst_cone <= rounding, f"an impulse left its friction cone by {worst_cone}"
sys.argv = [sys.argv[0], str(steps)]
penalty = runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ground_contact_humanoid.py"))
print(f"deepest corner {-lowest * 1e3:.2f} mm, deepest foot of the penalty ground {-penalty['lowest'] * 1e3:.2f} mm")
assert lowest > penalty["lowest"], "the corners sank deeper than the feet on the penalty ground"
print("self-check passed")
