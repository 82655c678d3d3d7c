"""CPU checker of mh_apparent_inertia_inverse_*: the inverse apparent inertia of K target bodies, column by column from the C oracle's
forward dynamics (MultiBodyResponseCalculator.java:1206-1338 restated as "the response is the forward dynamics of the test wrench alone,
at zero velocity, gravity and effort" -- tests/test_response.py pins that restatement), then the frame changes in numpy.

Without acceleration-source joints a column is `OracleModel.aba_bodies(q, 0, 0, g = 0, f_ext = unit wrench on a)`: rows of body_acc at the
targets.  With them it is `aba_locked(q, 0, 0, qdd_in = 0, ...)` for the joint accelerations and `rnea_bodies(q, 0, qdd+, g = 0)` for the
body accelerations they produce.  tests/test_apparent_inertia_cpu.py pins this file by facts that do not come from the same call."""
import numpy as np

ZERO_G = (0.0, 0.0, 0.0)


def skew(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def motion_into_frame(pose):
    """6 x 6 M: spatial acceleration (angular, linear) of the body-fixed frame -> that of a frame fixed in the body at `pose` (12 numbers,
    R row-major then p, frame -> body-fixed), no velocity terms: w' = R^T w, v' = R^T (v + w x p).  The wrench goes the other way with the
    transpose: (n, f)_body = M^T (n, f)_frame."""
    pose = np.asarray(pose, dtype=np.float64).reshape(12)
    R, p = pose[:9].reshape(3, 3), pose[9:]
    M = np.zeros((6, 6))
    M[:3, :3] = R.T
    M[3:, 3:] = R.T
    M[3:, :3] = -R.T @ skew(p)
    return M


def identity_poses(K):
    return np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (K, 1))


def body_frame_columns(om, q, joint, locked=None, second_route=False):
    """[B, n_joints, 6, 6]: entry [:, b, :, c] = change of the spatial acceleration of body b (body-fixed frame) per unit component c of a
    wrench on the successor body of `joint` (body-fixed frame).  second_route: forward dynamics, then the body accelerations from the
    Newton-Euler sweep instead of the forward dynamics' own (the route the locked case always takes)."""
    q = np.asarray(q, dtype=np.float64)
    B = q.shape[0]
    z = np.zeros((B, om.nv))
    out = np.zeros((B, om.n, 6, 6))
    for c in range(6):
        f = np.zeros((B, om.n, 6))
        f[:, joint, c] = 1.0
        if locked is not None and np.any(locked):
            qdd, _ = om.aba_locked(q, z, z, z, locked, ZERO_G, f)
            _, acc, _ = om.rnea_bodies(q, z, qdd, ZERO_G)
        elif second_route:
            qdd = om.aba(q, z, z, ZERO_G, f)
            _, acc, _ = om.rnea_bodies(q, z, qdd, ZERO_G)
        else:
            _, acc, _ = om.aba_bodies(q, z, z, ZERO_G, f)
        out[:, :, :, c] = acc
    return out


def apparent_inertia_inverse(om, q, targets, poses=None, coupled=False, locked=None, second_route=False):
    """What the device call returns in AoS: [B, K, 6, 6] (coupled=False) or [B, 6K, 6K]."""
    targets = [int(t) for t in targets]
    K = len(targets)
    poses = identity_poses(K) if poses is None else np.asarray(poses, dtype=np.float64).reshape(K, 12)
    M = [motion_into_frame(poses[k]) for k in range(K)]
    cols = {a: body_frame_columns(om, q, a, locked, second_route) for a in sorted(set(targets))}
    B = np.asarray(q).shape[0]
    if not coupled:
        W = np.zeros((B, K, 6, 6))
        for k, t in enumerate(targets):
            W[:, k] = M[k] @ cols[t][:, t] @ M[k].T
        return W
    W = np.zeros((B, 6 * K, 6 * K))
    for a, ta in enumerate(targets):
        for b, tb in enumerate(targets):
            W[:, 6 * b:6 * b + 6, 6 * a:6 * a + 6] = M[b] @ cols[ta][:, tb] @ M[a].T
    return W


def random_poses(rng, K):
    """K poses: a random rotation and an offset of up to 0.3 m each"""
    from mecano_amd import random_tools as rt
    out = np.zeros((K, 12))
    for k in range(K):
        out[k, :9] = rt.quaternionToMatrix(rt.nextQuaternion(rng)).reshape(9)
        out[k, 9:] = rng.uniform(-0.3, 0.3, 3)
    return out


def mass_matrix_conds(om, q):
    return np.array([np.linalg.cond(H, np.inf) for H in om.crba(np.asarray(q, dtype=np.float64))])


def bound_of(om, q, n_bodies, well_conditioned, u=2.0 ** -53):
    """Relative bound per configuration (times max(1, |ref|_inf) of that configuration): the project's standing 1e-10 on the models whose
    mass matrices are well conditioned by construction (arm, humanoid, ...), helpers.close_aba's 8 sqrt(8 n) cond_inf(H) u elsewhere --
    never below 1e-10, which is what forward dynamics is held to everywhere."""
    B = np.asarray(q).shape[0]
    if well_conditioned:
        return np.full(B, 1.0e-10)
    return np.maximum(1.0e-10, 8.0 * (8.0 * n_bodies) ** 0.5 * mass_matrix_conds(om, q) * u)


def close_rows(actual, ref, bounds, label=None):
    """max |actual - ref| per configuration <= bounds[row] * max(1, |ref|_inf of the row); logs the worst achieved / bound."""
    from helpers import record_parity
    actual, ref = np.asarray(actual, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert actual.shape == ref.shape, (actual.shape, ref.shape)
    B = ref.shape[0]
    err = np.abs(actual - ref).reshape(B, -1).max(axis=1)
    scale = np.maximum(1.0, np.abs(ref).reshape(B, -1).max(axis=1))
    ratio = err / (np.asarray(bounds) * scale)
    worst = int(np.argmax(ratio))
    print(f"{label}: worst err {err[worst]:.3e}, bound {bounds[worst] * scale[worst]:.3e}, ratio {ratio[worst]:.3e}")
    record_parity(float(ratio.max()), 1.0, (label or "W") + " err / bound")
    assert ratio.max() <= 1.0, f"{label}: row {worst}: err {err[worst]:.3e} > {bounds[worst] * scale[worst]:.3e}"
    return float(ratio.max())
