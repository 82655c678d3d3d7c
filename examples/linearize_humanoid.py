"""A, B of one explicit integration step x' = f(x, u) for 4 096 humanoids, x = (q, qd) in velocity-space coordinates, u = tau:
with qdd = aba(q, qd, tau) and the step qd' = qd + dt qdd, q' = q (+) dt qd',
    A = [[1 + dt^2 dqdd/dq,  dt (1 + dt dqdd/dqd)],        B = [[dt^2 Hinv],
         [    dt   dqdd/dq,       1 + dt dqdd/dqd ]],           [dt   Hinv]]
to first order in the step of q (the transport of a step across the update of a floating or spherical joint is left out).
Two launches of the library give every block.  Usage: python examples/linearize_humanoid.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mecano_amd import random_tools as rt  # noqa: E402
from mecano_amd.engine import HipModel  # noqa: E402

B, dt, g = 4096, 1.0e-3, (0.0, 0.0, -9.81)
system = rt.nextHumanoid(np.random.default_rng(43))
model = HipModel(system.toModelDesc())
q, qd, _, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(1), system, B))
qdd, dq, dv, Hinv = model.aba_derivatives(q, qd, tau, g)
eye = torch.eye(model.nv, dtype=q.dtype, device="cuda").expand(B, -1, -1)
bottom = torch.cat([dt * dq, eye + dt * dv], dim=2)
A = torch.cat([torch.cat([eye, torch.zeros_like(eye)], dim=2) + dt * bottom, bottom], dim=1)
Bm = torch.cat([dt * dt * Hinv, dt * Hinv], dim=1)
torch.cuda.synchronize()
print(f"A {tuple(A.shape)}, B {tuple(Bm.shape)}; |A - 1|_max = {float((A - torch.eye(2 * model.nv, device='cuda', dtype=q.dtype)).abs().max()):.3e}")
