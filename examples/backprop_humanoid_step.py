"""Trajectory optimisation by backpropagation through the library's own simulation step: torch.autograd across mecano_amd.autograd.step.

    python examples/backprop_humanoid_step.py [copies] [steps] [iterations]

4 096 copies of the committed floating-base humanoid (mecano_amd/models/humanoid30.json: a SixDoF root, so the configuration carries a
quaternion and q + dt qd is no integrator for it) start at rest in random poses and are rolled out for a short horizon with
(q, qd) <- step(q, qd, tau_t): forward dynamics, then the constant-acceleration integrator.  The loss is the mean squared distance of the
final joint angles to a target pose plus that of the final base height to its start; loss.backward() runs through every step -- one
mh_aba_integrate_vjp_* call per step between chart_cotangent and chart_pullback, no nv x nv matrix -- and plain gradient descent with a
backtracking step length updates the torque sequence [steps, copies, nv].  Ends with a self-check: the loss went down, and one component
of the gradient is compared with a central difference of the whole rollout (the disagreement is printed, not bounded).
Needs a built library and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd import autograd as mha
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel


def main(copies=4096, steps=8, iterations=5, seed=3, verbose=True):
    rng = np.random.default_rng(seed)
    desc = rt.modelDescFromJson("humanoid30")
    model, nv, dt, g = HipModel(desc), desc.nv, 0.005, (0.0, 0.0, -9.81)
    maps = mha.chart_maps(desc)
    angles = torch.tensor(maps["one_q"], device="cuda")          # the 1-DoF joints' entries of q
    height = int(maps["lin_q"][0][2])                            # z of the floating base
    q0 = rt.nextState(rng, rt.committedBenchmarkSystems()["humanoid30"], copies)[0]
    q0 = torch.tensor(q0, device="cuda")
    qd0 = torch.zeros((copies, nv), dtype=torch.float64, device="cuda")
    target = torch.tensor(rng.uniform(-1.0, 1.0, (1, len(maps["one_q"]))), device="cuda")
    tau = torch.zeros((steps, copies, nv), dtype=torch.float64, device="cuda", requires_grad=True)

    def rollout(torques):
        q, qd = q0, qd0
        for t in range(steps):
            q, qd = mha.step(model, dt, q, qd, torques[t].contiguous(), g)
        return ((q[:, angles] - target) ** 2).sum(dim=1).mean() + ((q[:, height] - q0[:, height]) ** 2).mean()

    losses, grad, lr = [], None, None
    for it in range(iterations + 1):
        loss = rollout(tau)
        losses.append(float(loss.detach()))
        (grad,) = torch.autograd.grad(loss, (tau,))
        if it == 0:  # one component against a central difference of the rollout, before the torques move
            t, b, j, h = steps // 2, copies // 3, nv // 2, 1.0e-3
            with torch.no_grad():
                e = torch.zeros_like(tau)
                e[t, b, j] = h
                fd = float((rollout(tau + e) - rollout(tau - e)) / (2.0 * h))
            ad = float(grad[t, b, j])
        if it < iterations:
            with torch.no_grad():  # backtracking: the first trial step would bring a loss linear in the torques to zero
                lr = (losses[-1] / float((grad ** 2).sum())) if lr is None else 2.0 * lr
                while not float(rollout(tau - lr * grad)) < losses[-1] and lr > 0.0:  # (a rollout that blew up is no descent either)
                    lr *= 0.5
                tau -= lr * grad
    disagreement = abs(ad - fd) / max(abs(fd), 1.0e-300)
    if verbose:
        print(f"{copies} humanoids, {steps} steps of {dt} s, {iterations} gradient-descent iterations on {tau.numel()} torques")
        print("loss: " + " -> ".join(f"{x:.6f}" for x in losses))
        print(f"d loss / d tau[{t}, {b}, {j}]: backward {ad:.6e}, central difference {fd:.6e}, relative disagreement {disagreement:.2e}")
    assert losses[-1] < losses[0], "the loss did not decrease"
    assert np.isfinite(disagreement)
    if verbose:
        print("self-check passed: the loss decreased")
    return losses, ad, fd


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:4]]
    main(*a)
