"""A contact between two moving bodies on the device: 4 096 collisions of two blocks, held against the closed form.

    python examples/two_body_contact.py [restitution]

Two blocks of masses m_a and m_b slide on parallel prismatic joints of the ground; block A catches up on block B.  The contact is
frictionless, its normal along the joint axes, pointing from block B (the base body) into block A (the target body).  A model holds one
mass per body, so the 4 096 collisions are 64 mass ratios over four decades -- 64 models, built through mecano_amd.multibody -- times 64
pairs of velocities each, one call of mh_contact_impulse_between_f64 (HipModel.contact_impulse_between) per model.  The restitution e
enters through v_normal = -e u_n, u_n the normal velocity of A relative to B before the impulse.  Newton's law of impact gives

    lambda = -(1 + e) u_n / (1 / m_a + 1 / m_b)        on A along the normal, its opposite on B,

so the total momentum m_a v_a + m_b v_b does not change, and at e = 0 both blocks leave with (m_a v_a + m_b v_b) / (m_a + m_b).  A rooted
contact (mh_contact_impulse_*) stops A against the ground's frame and leaves B alone: the momentum of the pair is not conserved.

It prints the worst deviation of the impulses, of the velocities and of the total momentum from the closed form, and checks them.
Needs a built library (python -m mecano_amd.build) and an MI355X."""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from mecano_amd.engine import HipModel
from mecano_amd.multibody import MultiBodySystem, PrismaticJoint, RigidBody

e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.4
RATIOS, PAIRS = 64, 64
X = (1.0, 0.0, 0.0)
BLOCK_A, BLOCK_B = 0, 1
NORMAL = (-1.0, 0.0, 0.0)  # from block B, ahead on the axis, into block A


def two_blocks(m_a, m_b):
    ground = RigidBody("ground")
    slide_a = PrismaticJoint("slide_a", ground, None, X)
    RigidBody("a", slide_a, np.diag([0.02, 0.03, 0.04]) * m_a, m_a)
    slide_b = PrismaticJoint("slide_b", ground, (np.eye(3), np.array([0.3, 0.1, 0.0])), X)
    RigidBody("b", slide_b, np.diag([0.03, 0.02, 0.05]) * m_b, m_b)
    return HipModel(MultiBodySystem.toMultiBodySystemInput(ground).toModelDesc())


rng = np.random.default_rng(0)
q = torch.tensor(rng.uniform(-0.2, 0.2, (PAIRS, 2)), device="cuda")
v_b = rng.uniform(-1.0, 1.0, PAIRS)
qd_host = np.stack([v_b + rng.uniform(0.1, 2.0, PAIRS), v_b], axis=1)  # A is the faster one: the blocks close
qd = torch.tensor(qd_host, device="cuda")
normals = torch.tensor(NORMAL, device="cuda", dtype=torch.float64).expand(PAIRS, 1, 3).contiguous()
u_n = -(qd_host[:, 0] - qd_host[:, 1])
v_normal = torch.tensor(-e * u_n[:, None], device="cuda")

worst_lam = worst_qd = worst_p = rooted_p = 0.0
for ratio in 10.0 ** np.linspace(-2.0, 2.0, RATIOS):
    m_a, m_b = float(np.sqrt(ratio)), float(1.0 / np.sqrt(ratio))
    model = two_blocks(m_a, m_b)
    qd_next, impulse, residual = model.contact_impulse_between(q, qd, [BLOCK_A], [BLOCK_B], [0.0], normals=normals, v_normal=v_normal)
    qd_rooted, _, _ = model.contact_impulse(q, qd, [BLOCK_A], [0.0], normals=normals, v_normal=v_normal)
    torch.cuda.synchronize()
    lam = -(1.0 + e) * u_n / (1.0 / m_a + 1.0 / m_b)
    want = np.stack([qd_host[:, 0] - lam / m_a, qd_host[:, 1] + lam / m_b], axis=1)
    got, imp = qd_next.cpu().numpy(), impulse.cpu().numpy()
    momentum = lambda v: m_a * v[:, 0] + m_b * v[:, 1]
    worst_lam = max(worst_lam, np.abs(imp[:, 0, 3:] - lam[:, None] * np.array(NORMAL)).max() / max(1.0, np.abs(lam).max()))
    worst_qd = max(worst_qd, np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    worst_p = max(worst_p, np.abs(momentum(got) - momentum(qd_host)).max() / max(1.0, np.abs(momentum(qd_host)).max()))
    rooted_p = max(rooted_p, np.abs(momentum(qd_rooted.cpu().numpy()) - momentum(qd_host)).max())
    if e == 0.0:
        common = momentum(qd_host) / (m_a + m_b)
        assert np.abs(got - common[:, None]).max() <= 1.0e-12 * max(1.0, np.abs(common).max()), "the blocks do not leave together"
    model.close()

print(f"{RATIOS * PAIRS} collisions, mass ratios 1e-2 .. 1e2, restitution {e}: worst deviation from the closed form {worst_lam:.1e} (impulse), "
      f"{worst_qd:.1e} (velocities), total momentum changed by {worst_p:.1e}; a rooted contact changes it by up to {rooted_p:.2f} kg m/s")
assert max(worst_lam, worst_qd, worst_p) <= 1.0e-12, "the collisions differ from the closed form"
assert rooted_p > 0.1
print("self-check passed")
