"""Identification by simulation error: fitting an unknown payload by descent on the inertial parameters through the forward dynamics.

    python examples/identify_by_simulation_error.py [samples] [iterations]

A 7-joint arm whose bodies have offset centres of mass (as in identify_parameters.py) carries an unknown payload in its last body.  The
"measurements" are the accelerations qdd = aba_parameters(q, qd, tau; pi_true) at random (q, qd, tau).  The ten numbers of the last body
are fitted by Adam on the mean of |autograd.aba_parameters(pi) - qdd|^2 through ONE shared parameter set: the batch's pi is
shared.expand(B, n, 10), so torch's own expand backward hands the optimiser the sum over the samples of what
HipModel.aba_parameters_vjp returns.  The accelerations are not linear in the parameters, so the regressor route of
identify_parameters.py does not apply; nothing goes to the host inside the loop.  Needs a built library and an MI355X."""
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


def with_payload(row, mass, at):
    """The ten numbers (m, c, J about the body-fixed origin) of a body with a point mass added at `at`."""
    m, c = row[0], row[1:4]
    out = row.copy()
    out[0] = m + mass
    out[1:4] = (m * c + mass * at) / (m + mass)
    x, y, z = at
    out[4:] += mass * np.array([y * y + z * z, -x * y, -x * z, x * x + z * z, -y * z, x * x + y * y])
    return out


def main(samples=4096, iterations=200, seed=7, verbose=True):
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

    def excite(count):
        q, qd, _, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(rng, system, count))
        return q, qd, tau

    def batch_of(last, count):
        return torch.cat([known, last[None]], 0).expand(count, n, 10).contiguous()

    q, qd, tau = excite(samples)
    measured = model.aba_parameters(q, qd, tau, batch_of(torch.tensor(true[-1], device="cuda"), samples), GRAVITY)

    def loss_of():
        predicted = mha.aba_parameters(model, q, qd, tau, batch_of(start + scale * z, samples), GRAVITY)
        return ((predicted - measured) ** 2).sum(1).mean()

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
        q2, qd2, tau2 = excite(samples)
        unseen = (model.aba_parameters(q2, qd2, tau2, batch_of(fitted, samples), GRAVITY)
                  - model.aba_parameters(q2, qd2, tau2, batch_of(torch.tensor(true[-1], device="cuda"), samples), GRAVITY)).abs().max()
        size = measured.abs().max()
    before, after, unseen, size = float(history[0]), float(history[-1]), float(unseen), float(size)
    if verbose:
        print(f"{samples} samples, {iterations} Adam steps on the last body's ten numbers")
        print(f"loss before {before:.3e}, after {after:.3e}; prediction error on {samples} new states {unseen:.2e}  (max |qdd| = {size:.1f})")
        print("last body, fitted / true:", np.array2string(fitted.detach().cpu().numpy() / true[-1], precision=3))
    return before, after, unseen


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 200)
