"""CPU checker of mh_mass_matrix_inverse_*: the inverse of the joint-space inertia matrix, column by column from the C oracle's forward
dynamics.  Column c is `OracleModel.aba(q, 0, e_c, g = 0)`: at zero velocity, gravity and external wrenches forward dynamics is
qdd = H^-1 tau (MultiBodyResponseCalculator.java:685-735 with :1206-1338 restated as "the response is the forward dynamics of the test
effort alone" -- tests/test_response.py pins that restatement).  With acceleration-source joints it is
`aba_locked(q, 0, e_c, qdd_in = 0, locked, g = 0)`, whose answer to an effort at a locked DoF is zero.  The oracle takes efforts and
returns accelerations in the model's DoF index map, so rows and columns are those of `OracleModel.crba`.
tests/test_mass_matrix_inverse_cpu.py pins this file by facts that do not come from the same call."""
import numpy as np

ZERO_G = (0.0, 0.0, 0.0)


def mass_matrix_inverse(om, q, columns=None, locked=None):
    """What the device call returns in AoS: [B, nv, nv], or [B, nv, K] for a list of K DoF indices (duplicates allowed)."""
    q = np.asarray(q, dtype=np.float64)
    B = q.shape[0]
    cols = list(range(om.nv)) if columns is None else [int(c) for c in columns]
    z = np.zeros((B, om.nv))
    out = np.zeros((B, om.nv, len(cols)))
    done = {}
    for k, c in enumerate(cols):
        if c not in done:
            e = np.zeros((B, om.nv))
            e[:, c] = 1.0
            if locked is not None and np.any(locked):
                done[c] = om.aba_locked(q, z, e, z, locked, ZERO_G)[0]
            else:
                done[c] = om.aba(q, z, e, ZERO_G)
        out[:, :, k] = done[c]
    return out


def locked_dofs(desc, locked):
    """DoF indices (index map) of the acceleration-source joints, and of the others."""
    ofs = np.concatenate([[0], np.cumsum([{0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}[int(t)] for t in desc.joint_type])])
    idx = np.asarray(desc.dof_indices, dtype=np.int64).reshape(-1)
    held = sorted(int(r) for j in range(desc.n_joints) if locked is not None and locked[j] for r in idx[ofs[j]:ofs[j + 1]])
    free = sorted(set(int(r) for r in idx[:ofs[-1]]) - set(held))
    return held, free


def joint_dofs(desc, joint):
    """DoF indices (index map) of one joint of the description"""
    ofs = np.concatenate([[0], np.cumsum([{0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}[int(t)] for t in desc.joint_type])])
    return [int(r) for r in np.asarray(desc.dof_indices, dtype=np.int64).reshape(-1)[ofs[joint]:ofs[joint + 1]]]


def column_list(desc, seed=1):
    """A list for the device tests: for the first multi-DoF joint a strict subset of its DoFs, then DoFs of other joints in no order,
    one of them named twice."""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(desc.n_joints):
        d = joint_dofs(desc, j)
        if len(d) >= 3:
            cols += [d[-1], d[1]]
            break
    cols += [int(c) for c in rng.integers(0, desc.nv, 5)]
    cols.append(cols[len(cols) // 2])
    return cols
