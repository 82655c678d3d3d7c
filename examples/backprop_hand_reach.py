"""Reaching a point in space by backpropagation through the batched forward dynamics AND the kinematics: torch.autograd across
mecano_amd.autograd.aba and mecano_amd.autograd.body_poses.  The Cartesian twin of examples/backprop_arm_reach.py.

    python examples/backprop_hand_reach.py [copies] [steps] [iterations]

4 096 copies of the committed 7-joint arm (mecano_amd/models/arm7.json; all joints revolute, so q + dt qd is the whole integrator and
stays in torch) start at rest in random poses and are rolled out for a short horizon with semi-implicit Euler, qd' = qd + dt aba(q, qd,
tau_t), q' = q + dt qd'.  The loss is the mean squared distance of a tool point -- a frame fixed in the last body, 0.12 m off its
body-fixed frame and turned against it -- to a target POINT in the root body frame, read from autograd.body_poses at the last step, plus a
small penalty on the last velocities.  loss.backward() carries the gradient from the hand position back to q with one mh_body_poses_vjp_*
call (nv numbers per copy, no Jacobian) and then through every step with one mh_aba_vjp_* call each; plain gradient descent with a
backtracking step length updates the torque sequence [steps, copies, nv].  Ends with the twin's self-check: the loss went down, and one
component of the gradient is compared with a central difference of the whole rollout (the disagreement is printed, not bounded).
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
    desc = rt.modelDescFromJson("arm7")
    model, nv, dt, g = HipModel(desc), desc.nv, 0.01, (0.0, 0.0, -9.81)
    q0 = torch.tensor(rng.uniform(-1.0, 1.0, (copies, desc.nq)), device="cuda")
    qd0 = torch.zeros((copies, nv), dtype=torch.float64, device="cuda")
    tool_body = [desc.n_joints - 1]
    c, s = np.cos(0.4), np.sin(0.4)
    tool_pose = np.array([[c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c, 0.03, 0.0, 0.12]])  # turned about y, 0.12 m along z
    # a target the arms can reach: where the tool point of one random pose is
    point = model.body_poses(torch.tensor(rng.uniform(-1.0, 1.0, (1, desc.nq)), device="cuda"), tool_body, tool_pose)[:, 0, 9:]
    tau = torch.zeros((steps, copies, nv), dtype=torch.float64, device="cuda", requires_grad=True)

    def rollout(torques):
        q, qd = q0, qd0
        for t in range(steps):
            qd = qd + dt * mha.aba(model, q, qd, torques[t].contiguous(), g)
            q = q + dt * qd
        hand = mha.body_poses(model, q.contiguous(), tool_body, tool_pose)[:, 0, 9:]
        return ((hand - point) ** 2).sum(dim=1).mean() + 1.0e-2 * (qd ** 2).sum(dim=1).mean()

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
                while float(rollout(tau - lr * grad)) >= losses[-1] and lr > 0.0:
                    lr *= 0.5
                tau -= lr * grad
    disagreement = abs(ad - fd) / max(abs(fd), 1.0e-300)
    if verbose:
        print(f"{copies} arms, {steps} steps of {dt} s, {iterations} gradient-descent iterations on {tau.numel()} torques")
        print("loss (squared distance of the tool point to the target point): " + " -> ".join(f"{x:.6f}" for x in losses))
        print(f"d loss / d tau[{t}, {b}, {j}]: backward {ad:.6e}, central difference {fd:.6e}, relative disagreement {disagreement:.2e}")
    assert losses[-1] < losses[0], "the loss did not decrease"
    assert np.isfinite(disagreement)
    if verbose:
        print("self-check passed: the loss decreased")
    return losses, ad, fd


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:4]]
    main(*a)
