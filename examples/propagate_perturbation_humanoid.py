"""A perturbation of the initial state carried through a rollout in forward mode: one mh_aba_integrate_jvp_* call per step.

    python examples/propagate_perturbation_humanoid.py [copies] [steps]

4 096 copies of the committed floating-base humanoid (mecano_amd/models/humanoid30.json: a SixDoF root, so the configuration carries a
quaternion and its perturbation lives in velocity space) start in random states and are rolled out under constant random torques with
(q, qd) <- step(q, qd, tau).  Beside the rollout a direction (dq, dqd) of the initial state -- dq a velocity-space step of
configuration_add -- is pushed through every step with step_jvp: (dq, dqd) <- A (dq, dqd) without A, no nv x nv matrix anywhere.  Nothing
leaves the device inside the loop.  Ends with a self-check: two more rollouts start at q0 (+) (+-h dq0), qd0 +- h dqd0, and the central
difference of their final states -- taken in the chart at the unperturbed final configuration with configuration_difference -- is
compared with the propagated direction (the distance is printed, and held to the size of the difference's own truncation error).
Needs a built library and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel


def main(copies=4096, steps=16, seed=3, verbose=True):
    rng = np.random.default_rng(seed)
    desc = rt.modelDescFromJson("humanoid30")
    model, nv, dt, g, h = HipModel(desc), desc.nv, 0.002, (0.0, 0.0, -9.81), 1.0e-5
    model.reserve(copies)
    q0, qd0, _, _ = (torch.tensor(x, device="cuda") for x in rt.nextState(rng, rt.committedBenchmarkSystems()["humanoid30"], copies))
    tau = torch.tensor(rng.uniform(-1.0, 1.0, (copies, nv)), device="cuda")
    dq0, dqd0 = (torch.tensor(rng.uniform(-1.0, 1.0, (copies, nv)), device="cuda") for _ in range(2))

    def rollout(q, qd, dq=None, dqd=None):
        for _ in range(steps):
            if dq is not None:  # the tangent first: it is taken at the state the step starts from
                _, _, dq, dqd = model.step_jvp(dt, q, qd, tau, dq, dqd, None, g, out=(None, None, torch.empty_like(dq), torch.empty_like(dqd)))
            q, qd, _ = model.step(dt, q, qd, tau, g)
        return q, qd, dq, dqd

    q, qd, dq, dqd = rollout(q0, qd0, dq0, dqd0)
    ends = [rollout(model.configuration_add(q0, s * h * dq0), qd0 + s * h * dqd0)[:2] for s in (1.0, -1.0)]
    fd_q = (model.configuration_difference(q, ends[0][0]) - model.configuration_difference(q, ends[1][0])) / (2.0 * h)
    fd_qd = (ends[0][1] - ends[1][1]) / (2.0 * h)
    err_q, err_qd = float((dq - fd_q).abs().max()), float((dqd - fd_qd).abs().max())
    size_q, size_qd = float(dq.abs().max()), float(dqd.abs().max())
    if verbose:
        print(f"{copies} humanoids, {steps} steps of {dt} s: a direction of the initial state pushed through the rollout by step_jvp")
        print(f"dq_T:  |.| up to {size_q:.4g}, distance to the central difference (h = {h:g}) {err_q:.3e}")
        print(f"dqd_T: |.| up to {size_qd:.4g}, distance to the central difference {err_qd:.3e}")
    assert np.isfinite(err_q) and np.isfinite(err_qd)
    # the difference quotient's own error: truncation h^2 |x'''| and cancellation u |x| / h, both far below 1e-4 of the tangent here
    assert err_q <= 1.0e-4 * max(1.0, size_q) and err_qd <= 1.0e-4 * max(1.0, size_qd), "the propagated direction is not the derivative"
    if verbose:
        print("self-check passed: the propagated direction is the derivative of the rollout")
    return err_q, err_qd


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]]
    main(*a)
