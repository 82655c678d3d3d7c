"""Joint limits beside frictional ground contact, without leaving the device: the 4096 limp humanoids of
examples/frictional_contact_humanoid.py again, with ranges on their hips, knees and elbows, so that they no longer fold through themselves.

    python examples/joint_limits_humanoid.py [steps]

The same velocity-level time-stepping scheme, with two unilateral blocks per step: the eight sole corners (mh_contact_impulse_f64) and the
ten limited joints (mh_joint_limit_impulse_f64).  Each call solves its own block alone; the step alternates them twice, each on the free
velocity plus the other's change of velocity -- block Gauss-Seidel on the joint dual problem -- and both are warm-started by their own
impulses (the outputs are their own warm starts).  The limits go last: with erp = 1 / dt a closed row asks for exactly "do not cross in this
step", and a row closes MARGIN before its limit, further than any joint here travels in one step.  Nothing inside the loop reads a value
back to the host.

It ends with a relational self-check: no listed joint ever ended a step more than TOLERANCE outside its range; no limit ever pulled (every
s_i impulse_i >= 0 to rounding); and the same run without the limit call does leave the ranges, by far more -- so the first check can fail.
Needs a built library (python -m mecano_amd.build) and an MI355X."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
B, dt, g = 4096, 1.0e-3, 9.81
MU, BETA, COMPLIANCE, SWEEPS, ROUNDS = 0.7, 0.2, 1.0e-4, 50, 2
JOINT_DAMPING = 0.5
FEET = [6, 12]
TARGETS = [FEET[0]] * 4 + [FEET[1]] * 4
K = len(TARGETS)
CORNERS = np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (K, 1))
for k in range(K):
    CORNERS[k, 9:] = (0.1 if k & 1 else -0.1, 0.05 if k & 2 else -0.05, 0.0)
# joints 1-6 / 7-12 are the legs (hip x 3, knee, ankle x 2), 16-19 / 20-23 the arms (shoulder x 2, elbow, wrist)
HIPS, KNEES, ELBOWS = [1, 2, 3, 7, 8, 9], [4, 10], [18, 22]
LIMITED = HIPS + KNEES + ELBOWS
LOWER = np.array([-0.6] * len(HIPS) + [0.0] * len(KNEES) + [0.0] * len(ELBOWS))
UPPER = np.array([0.6] * len(HIPS) + [2.0] * len(KNEES) + [2.2] * len(ELBOWS))
MARGIN, ERP, LIMIT_COMPLIANCE = 0.1, 1.0 / dt, 0.0  # a joint would have to turn at 100 rad/s to pass the margin in one step
TOLERANCE = 1.0e-3                                  # rad a joint may end a step outside its range

system = rt.nextHumanoid(np.random.default_rng(43))
desc = system.toModelDesc()
model = HipModel(desc)
model.reserve(B)
L = len(LIMITED)
# revolute joint j owns one configuration and one DoF index; the floating joint in front of them takes 7 and 6
cfg_of = [int(desc.cfg_indices[7 + (j - 1)]) for j in LIMITED]
lower, upper = (torch.tensor(x, device="cuda") for x in (LOWER, UPPER))
pelvis_z = int(desc.cfg_indices[6])
joint_damping = torch.full((desc.nv,), JOINT_DAMPING, dtype=torch.float64, device="cuda")
joint_damping[[int(i) for i in desc.dof_indices[:6]]] = 0.0


def simulate(with_limits):
    """(worst excess over the run [rad], least s_i impulse_i, largest |limit impulse|, robots that touched the ground)"""
    q, qd, _, _ = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(0), system, B))
    qd.zero_()
    # the limited joints start inside their ranges: the random angle, brought to the middle 80 % of the range
    q[:, cfg_of] = lower + (upper - lower) * (0.1 + 0.8 * (0.5 + 0.5 * torch.sin(q[:, cfg_of])))
    q[:, pelvis_z] += 0.02 - model.body_poses(q, TARGETS, CORNERS)[:, :, 11].amin(dim=1)
    corner = torch.empty((B, K, 12), dtype=torch.float64, device="cuda")
    v_contact, v_limit = torch.empty_like(qd), torch.empty_like(qd)
    impulse = torch.zeros((B, K, 6), dtype=torch.float64, device="cuda")
    limit_impulse = torch.zeros((B, L), dtype=torch.float64, device="cuda")
    residual, limit_residual = (torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(2))
    excess = torch.zeros((), dtype=torch.float64, device="cuda")
    least_push = torch.full((), float("inf"), dtype=torch.float64, device="cuda")
    largest = torch.zeros((), dtype=torch.float64, device="cuda")
    touched = torch.zeros(B, dtype=torch.bool, device="cuda")
    for _ in range(steps):
        model.body_poses(q, TARGETS, CORNERS, out=corner)
        height = corner[:, :, 11]
        active = (height <= 0.0).to(torch.int32)
        v_normal = (-BETA / dt * height).contiguous()
        v_free = qd + dt * model.aba(q, qd, -joint_damping * qd, (0.0, 0.0, -g))
        dv_limit = torch.zeros_like(qd)
        for _ in range(ROUNDS if with_limits else 1):
            model.contact_impulse(q, v_free + dv_limit, TARGETS, [MU] * K, CORNERS, None, active, v_normal, COMPLIANCE, SWEEPS, init=impulse,
                                  out=(v_contact, impulse, residual))
            qd = v_contact
            if with_limits:
                dv_contact = v_contact - (v_free + dv_limit)
                model.joint_limit_impulse(q, v_free + dv_contact, LIMITED, LOWER, UPPER, MARGIN, ERP, LIMIT_COMPLIANCE, SWEEPS, init=limit_impulse,
                                          out=(v_limit, limit_impulse, limit_residual))
                dv_limit = v_limit - (v_free + dv_contact)
                qd = v_limit
        if with_limits:  # the sides as the call saw them, before the step moves q
            angle = q[:, cfg_of]
            side = torch.where(angle - lower <= upper - angle, 1.0, -1.0)
            least_push = torch.minimum(least_push, (side * limit_impulse).amin())
            largest = torch.maximum(largest, limit_impulse.abs().amax())
        qd = qd.clone()
        model.configuration_add(q, dt * qd, out=q)
        angle = q[:, cfg_of]
        excess = torch.maximum(excess, torch.maximum(lower - angle, angle - upper).amax())
        touched |= active.any(dim=1)
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(qd).all(), "the state blew up"
    return float(excess), float(least_push), float(largest), int(touched.sum())


excess, least_push, largest, landed = simulate(True)
print(f"{steps} steps of {B} humanoids with {L} joint ranges: {landed} touched the ground, worst excess over a range {excess:.2e} rad, "
      f"largest limit impulse {largest:.3f} N m s, least s * impulse {least_push:.2e}")
assert excess <= TOLERANCE, f"a listed joint ended a step {excess} rad outside its range"
assert least_push >= -1.0e-12 * max(1.0, largest), f"a limit pulled: s * impulse = {least_push}"
free_excess, _, _, _ = simulate(False)
print(f"without the limit call the same joints leave their ranges by up to {free_excess:.3f} rad")
assert free_excess > 100.0 * TOLERANCE and (largest > 0.0 or steps < 50), "the run without limits stayed inside the ranges: the check could not fail"
print("self-check passed")
