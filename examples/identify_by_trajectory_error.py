"""Identification by trajectory error: fitting an unknown payload from measured states after a rollout, by backpropagation through the
simulation steps with respect to the state AND the inertial parameters.

    python examples/identify_by_trajectory_error.py [samples] [horizon] [iterations]

4 096 seven-joint arms whose bodies have offset centres of mass (as in identify_by_simulation_error.py) carry the same unknown payload
in their last body.  Every arm starts from its own random (q, qd) under its own constant efforts; the "measurements" are the states
(q_H, qd_H) after H semi-implicit steps of the true robot.  The ten numbers of the last body are fitted by Adam on the mean squared
distance of the predicted to the measured final states, through H calls of autograd.step_parameters: every step's backward is ONE
HipModel.aba_parameters_state_vjp -- the gradients with respect to q, qd and pi of the same step from one adjoint sweep -- and the
integrator's own.  identify_by_simulation_error.py needs measured accelerations; here the gradient has to travel through the states of
H steps, which the parameter-only gradients cannot carry.  The batch's pi is shared.expand(B, n, 10), so torch's expand backward sums
the rows; nothing goes to the host inside the loop.  Needs a built library and an MI355X."""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mecano_amd import autograd as mha
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel
from mecano_amd.multibody import MultiBodySystem

GRAVITY = (0.0, 0.0, -9.81)
DT = 0.005


def with_payload(row, mass, at):
    """The ten numbers (m, c, J about the body-fixed origin) of a body with a point mass added at `at`."""
    m, c = row[0], row[1:4]
    out = row.copy()
    out[0] = m + mass
    out[1:4] = (m * c + mass * at) / (m + mass)
    x, y, z = at
    out[4:] += mass * np.array([y * y + z * z, -x * y, -x * z, x * x + z * z, -y * z, x * x + y * y])
    return out


def main(samples=4096, horizon=20, iterations=100, seed=7, verbose=True):
    rng = np.random.default_rng(seed)
    system = MultiBodySystem.toMultiBodySystemInput(rt.nextJointChain(rng, 7, ("revolute",))[0].getPredecessor())
    desc = system.toModelDesc()
    desc = dataclasses.replace(desc, inertia_com=rng.uniform(-0.2, 0.2, 3 * desc.n_joints))  # Mecano's generators leave the offsets at zero
    model = HipModel(desc)
    n = desc.n_joints
    nominal = model.inertial_parameters()                                     # what the description says: no payload
    true = nominal.copy()
    true[-1] = with_payload(nominal[-1], 0.4 * nominal[-1, 0], np.array([0.05, -0.03, 0.08]))
    known = torch.tensor(nominal[:-1], device="cuda")                         # the other bodies are known
    scale = torch.tensor(np.abs(nominal[-1]) + 0.05 * np.abs(nominal[-1]).max(), device="cuda")
    start = torch.tensor(nominal[-1], device="cuda")
    z = torch.zeros(10, dtype=torch.float64, device="cuda", requires_grad=True)  # the last body, in units of its nominal numbers
    q0, qd0, _, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(rng, system, samples))

    def rollout(last):
        pi = torch.cat([known, last[None]], 0).expand(samples, n, 10).contiguous()
        q, qd = q0, qd0
        for _ in range(horizon):
            q, qd = mha.step_parameters(model, DT, q, qd, tau, pi, GRAVITY)
        return q, qd

    with torch.no_grad():
        q_meas, qd_meas = rollout(torch.tensor(true[-1], device="cuda"))

    def loss_of():
        q, qd = rollout(start + scale * z)
        T = DT * horizon  # a constant error of the acceleration moves q by T^2 / 2 and qd by T: both terms in units of its square
        return (((q - q_meas) ** 2).sum(1) / T ** 4 + ((qd - qd_meas) ** 2).sum(1) / T ** 2).mean()

    optimiser = torch.optim.Adam([z], lr=0.02)
    history = torch.zeros(iterations + 1, dtype=torch.float64, device="cuda")
    for it in range(iterations):
        optimiser.zero_grad(set_to_none=True)
        loss = loss_of()
        history[it] = loss.detach()
        loss.backward()
        optimiser.step()
    with torch.no_grad():
        history[iterations] = loss_of()
        fitted = start + scale * z
    before, after = float(history[0]), float(history[-1])
    if verbose:
        print(f"{samples} arms, {horizon} steps of {DT} s, {iterations} Adam steps on the last body's ten numbers")
        print(f"loss before {before:.3e}, after {after:.3e}")
        print("last body, fitted / true:", np.array2string(fitted.detach().cpu().numpy() / true[-1], precision=3))
    return before, after


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:4]]
    main(*args)
