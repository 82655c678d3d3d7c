"""A, B of the simulation step the library takes, x' = step(x, u) for 4 096 humanoids: x = (q, qd), u = tau, dx' = A dx + B du with dq and
dq' velocity-space steps in the chart of configuration_add / configuration_difference (the transport across the update of the floating
joint included) -- one call, HipModel.step_derivatives.  Self-check: step(x (+) eps e) (-) step(x) against eps A e for one rotational
column of the floating joint, eps = 1e-6, within 2e-5 cond_inf(H) max(1, |A|_inf).  Usage: python examples/linearize_humanoid.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mecano_amd import random_tools as rt  # noqa: E402
from mecano_amd.engine import HipModel  # noqa: E402

B, dt, g, eps = 4096, 1.0e-3, (0.0, 0.0, -9.81), 1.0e-6
system = rt.nextHumanoid(np.random.default_rng(43))
desc = system.toModelDesc()
model = HipModel(desc)
q, qd, _, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(1), system, B))
qdd, q_next, qd_next, A, Bm = model.step_derivatives(dt, q, qd, tau, g)
torch.cuda.synchronize()
eye = torch.eye(2 * model.nv, device="cuda", dtype=q.dtype)
print(f"A {tuple(A.shape)}, B {tuple(Bm.shape)}; |A - 1|_max = {float((A - eye).abs().max()):.3e}")

floating = [j for j in range(desc.n_joints) if int(desc.joint_type[j]) == 2][0]  # MH_JOINT_SIXDOF
ofs = sum({0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}[int(t)] for t in desc.joint_type[:floating])
col = int(desc.dof_indices[ofs + 1])  # the joint's second rotational DoF
e = torch.zeros_like(qd)
e[:, col] = eps
q_eps = model.configuration_add(q, e)
q_next_eps, qd_next_eps = model.integrate(dt, q_eps, qd, model.aba(q_eps, qd, tau, g))
lhs = torch.cat([model.configuration_difference(q_next, q_next_eps), qd_next_eps - qd_next], dim=1) / eps
residual = (lhs - A[:, :, col]).abs().amax(dim=1)
cond = torch.linalg.cond(model.crba(q), p=float("inf"))
bound = 2.0e-5 * cond * A.abs().amax(dim=(1, 2)).clamp(min=1.0)
worst = float((residual / bound).max())
print(f"self-check, column {col} of the floating joint: worst residual {float(residual.max()):.3e}, worst residual / bound {worst:.3e}"
      f" ({'within' if worst <= 1.0 else 'OUTSIDE'} the bound)")
