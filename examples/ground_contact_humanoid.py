"""Ground contact without leaving the device: 4096 limp 30-DoF humanoids dropped onto their feet.

    python examples/ground_contact_humanoid.py [steps]

Every step computes, on the device, the poses of the two feet in the world (mh_body_poses_f64) and their Jacobians (mh_geometric_jacobian_f64:
J qd is the twist of the foot in its own frame), turns foot height and foot velocity into a spring-damper force in the world, rotates it
into the body-fixed frame of the foot -- the frame f_ext is expressed in -- and takes one step of forward dynamics and integration
(mh_aba_integrate_f64).  Nothing inside the loop reads a value back to the host.  A light viscous damping at the joints stands in for
the passive dissipation of a real mechanism.

It ends with a self-check: no robot holds more mechanical energy (kinetic, gravitational, elastic) than it started with, up to
ENERGY_SLACK of its weight times one metre -- the ground and the joints only dissipate -- and no foot ever sank deeper below the ground
than a spring holds when it alone stores what the whole weight releases over the fall available to these robots: sqrt(2 W FALL / k).  The
random humanoid is metres tall and starts in any attitude; FALL is taken from the batch itself, twice the largest initial distance in
height between a robot's centre of mass and its lower foot (down onto the foot and as far again swinging through below it): a generous
scale that a contact model gone wrong (a wrong frame, a wrong sign) exceeds at once, not a tight bound.
Needs a built library (python -m mecano_amd.build) and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
B, dt, g = 4096, 1.0e-3, 9.81
STIFFNESS, DAMPING, FRICTION = 5.0e4, 150.0, 50.0  # N/m, N s/m normal, N s/m tangential (viscous)
JOINT_DAMPING = 0.5                                 # N m s/rad
ENERGY_SLACK = 0.05                                 # share of (total weight x 1 m)
FEET = [6, 12]                                      # last joints of the two leg chains

system = rt.nextHumanoid(np.random.default_rng(43))
desc = system.toModelDesc()
model = HipModel(desc)
model.reserve(B)
mass = torch.tensor(np.asarray(desc.inertia_mass), device="cuda")
weight = float(mass.sum()) * g

q, qd, _, _ = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(0), system, B))
qd.zero_()
pelvis_z = int(desc.cfg_indices[6])  # the floating joint's configuration is (qx, qy, qz, qs, x, y, z)
# every robot starts with its lower foot 2 cm above the ground (z = 0)
q[:, pelvis_z] += 0.02 - model.body_poses(q, FEET)[:, :, 11].amin(dim=1)
com_height = (model.body_poses(q)[:, :, 11] * mass).sum(dim=1) / mass.sum()  # the body-fixed frames sit at the centres of mass
FALL = 2.0 * float((com_height - 0.02).abs().max())
MAX_DEPTH = (2.0 * weight * FALL / STIFFNESS) ** 0.5

foot_pose = torch.empty((B, 2, 12), dtype=torch.float64, device="cuda")
foot_J = torch.empty((B, 12, desc.nv), dtype=torch.float64, device="cuda")
f_ext = torch.zeros((B, desc.n_joints, 6), dtype=torch.float64, device="cuda")
friction = torch.tensor([FRICTION, FRICTION, DAMPING], device="cuda")
feet = torch.tensor(FEET, device="cuda")
joint_damping = torch.full((desc.nv,), JOINT_DAMPING, dtype=torch.float64, device="cuda")
joint_damping[[int(i) for i in desc.dof_indices[:6]]] = 0.0  # the floating base is free


def contact_forces():
    """(height of the feet [B, 2], force on them in the world [B, 2, 3]); f_ext gets the force in the feet's own frames"""
    model.body_poses(q, FEET, out=foot_pose)
    model.geometric_jacobian(q, FEET, out=foot_J)
    R = foot_pose[:, :, :9].view(B, 2, 3, 3)
    height = foot_pose[:, :, 11]
    twist = torch.einsum("bij,bj->bi", foot_J, qd).view(B, 2, 6)
    velocity = torch.einsum("bkij,bkj->bki", R, twist[:, :, 3:])  # of the foot frame's origin, in the world
    force = -friction * velocity
    force[:, :, 2] -= STIFFNESS * height
    force = torch.where((height < 0.0)[:, :, None], force, torch.zeros_like(force))
    f_ext[:, feet, 3:] = torch.einsum("bkji,bkj->bki", R, force)  # R^T f: the body-fixed frame sits at the centre of mass, the force acts there
    return height, force


def energy():
    """kinetic + gravitational + elastic, per robot: the body-fixed frames sit at the centres of mass"""
    H = model.crba(q)
    kinetic = 0.5 * torch.einsum("bi,bij,bj->b", qd, H, qd)
    potential = g * (model.body_poses(q)[:, :, 11] * mass).sum(dim=1)
    depth = torch.clamp(-model.body_poses(q, FEET)[:, :, 11], min=0.0)
    return kinetic + potential + 0.5 * STIFFNESS * (depth * depth).sum(dim=1)


energy_start = energy()
lowest = torch.full((), float("inf"), dtype=torch.float64, device="cuda")
touched = torch.zeros(B, dtype=torch.bool, device="cuda")
for _ in range(steps):
    height, _ = contact_forces()
    lowest = torch.minimum(lowest, height.amin())
    touched |= (height < 0.0).any(dim=1)
    model.step(dt, q, qd, -joint_damping * qd, (0.0, 0.0, -g), f_ext, inplace=True)
torch.cuda.synchronize()

gain = float((energy() - energy_start).max())
lowest, landed = float(lowest), int(touched.sum())
print(f"{steps} steps of {B} humanoids: {landed} touched the ground, deepest foot {-lowest * 1e3:.2f} mm below it, "
      f"(limit {MAX_DEPTH * 1e3:.1f} mm for a fall of {FALL:.2f} m), largest energy gain {gain:.3f} J (weight x 1 m = {weight:.1f} J)")
assert torch.isfinite(q).all() and torch.isfinite(qd).all(), "the state blew up"
assert landed == B or steps < 200, "some robot never reached the ground"
assert lowest >= -MAX_DEPTH, f"a foot sank {-lowest:.4f} m below the ground (limit {MAX_DEPTH} m)"
assert gain <= ENERGY_SLACK * weight, f"a robot gained {gain:.3f} J (limit {ENERGY_SLACK * weight:.3f} J)"
print("self-check passed")
