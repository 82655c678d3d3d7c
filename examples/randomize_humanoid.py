"""Domain randomisation: 4096 humanoids of one topology whose link masses and centres of mass differ, falling under gravity.

    python examples/randomize_humanoid.py [steps]

Every robot brings its own ten inertial numbers per body (HipModel.inertial_parameters() of the nominal robot, perturbed); each step is
aba_parameters (forward dynamics with per-configuration parameters, mh_aba_parameters_f64) followed by integrate.  The state never leaves
the GPU, and no model handle is created per robot.  Needs a built library (python -m mecano_amd.build) and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel

B, dt = 4096, 1.0e-3
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000  # one second
system = rt.nextHumanoid(np.random.default_rng(43))
desc = system.toModelDesc()
model = HipModel(desc)
rng = np.random.default_rng(7)

pi = np.broadcast_to(model.inertial_parameters(), (B, desc.n_joints, 10)).copy()
m, c = pi[:, :, 0].copy(), pi[:, :, 1:4].copy()
J = np.zeros((B, desc.n_joints, 3, 3))
for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
    J[..., a, b] = J[..., b, a] = pi[:, :, 4 + k]
shift = lambda mass, com: mass[..., None, None] * ((com ** 2).sum(-1)[..., None, None] * np.eye(3) - com[..., :, None] * com[..., None, :])
Jc = J - shift(m, c)                                   # central inertia of the nominal link
m2 = m * rng.uniform(0.8, 1.25, m.shape)               # +- 25 % of mass per link and robot
c2 = c + rng.uniform(-0.02, 0.02, c.shape)             # centre of mass moved by up to 2 cm per axis
J2 = Jc * (m2 / np.where(m > 0, m, 1.0))[..., None, None] + shift(m2, c2)  # same shape of the link, back about the body-fixed origin
pi[:, :, 0], pi[:, :, 1:4] = m2, c2
for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
    pi[:, :, 4 + k] = J2[..., a, b]

state = rt.nextState(np.random.default_rng(0), system, 1)
q = torch.tensor(np.repeat(state[0], B, axis=0), device="cuda")   # every robot starts in the same pose, at rest
qd = torch.zeros((B, desc.nv), dtype=torch.float64, device="cuda")
tau = torch.zeros_like(qd)                                        # limp robots
pi_d = torch.tensor(pi, device="cuda")
qdd = torch.empty_like(qd)
pelvis_z = list(system.getJointMatrixIndexProvider().getJointConfigurationIndices(system.getJointMatrixIndexProvider().getIndexedJointsInOrder()[0]))[6]
z0 = q[:, pelvis_z].clone()
for _ in range(steps):
    model.aba_parameters(q, qd, tau, pi_d, (0.0, 0.0, -9.81), out=qdd)
    q, qd = model.integrate(dt, q, qd, qdd)[:2]
torch.cuda.synchronize()
drop = (q[:, pelvis_z] - z0).cpu().numpy()
print(f"{B} randomised humanoids after {steps * dt:.2f} s: pelvis height change {drop.mean():+.4f} m on average, "
      f"spread {drop.std():.2e} m (min {drop.min():+.4f}, max {drop.max():+.4f})")
