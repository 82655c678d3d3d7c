"""Times mh_contact_impulse_* beside what a caller issues without it for the same result -- mh_rnea_bodies (twists), mh_body_poses (the
normals in the target frames), mh_apparent_inertia_inverse (COUPLED), the same projected Gauss-Seidel sweeps written in batched torch, mh_aba
at rest with the impulses as wrenches, an add -- in the same session, on the 30-DoF humanoid: K = 2, 4 and 8 contact points (both feet; feet
and hands; four points per foot) at 10, 50 and 200 sweeps, fp64 and fp32, AoS and SoA.  Identity target poses and the default normal, so
that the composition's glue is as light as it gets.  HIP events around `reps` back-to-back calls after a warm-up, the candidates
alternated over three rounds; prints the median per call with its spread, the ratio, the solve kernel alone (the call minus its reused
launches, each timed alone in the same rounds) and, for scale only -- it solves a different problem -- mh_constraint_impulse_* with the same
points as POINT rows.  Where both are possible the LDS-resident and the streamed solve are timed against each other.
Usage: python tools/measure_contact_dynamics.py [B ...] (default 4096 262144); writes profiles/contact_dynamics_rates.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {2: [6, 12], 4: [6, 12, 19, 23], 8: [6, 6, 6, 6, 12, 12, 12, 12]}
SWEEPS = (10, 50, 200)
MU, EPS = 0.5, 1.0e-6
ZERO_G = (0.0, 0.0, 0.0)


def corner_poses(K):
    out = np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (K, 1))
    if K == 8:
        for k in range(K):
            out[k, 9:] = (0.1 if k & 1 else -0.1, 0.05 if k & 2 else -0.05, -0.05)
    return out


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in sys.argv[1:]] or [4096, 262144]
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    lib = _lib.load()
    nv, n = desc.nv, desc.n_joints
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def timed(cands, reps, rounds=3):
        times = {k: [] for k in cands}
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in cands.items():
                r = reps(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(r):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / r)
        return times

    say(f"model: humanoid, {n} joints, nv = {nv}, kernel variant: {hm.kernel_variant}; mu = {MU}, compliance = {EPS}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    for B in batches:
        hm.reserve(B)
        q0, qd0, _, _ = rt.nextState(np.random.default_rng(1), sys_, 4096)
        tile = lambda x, dt: torch.tensor(x, device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous()
        for dt, prec in ((torch.float64, "fp64"), (torch.float32, "fp32")):
            for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                aos = layout == _lib.LAYOUT_AOS
                lay = lambda x: x if aos else x.reshape(B, -1).t().contiguous()
                q, qd = lay(tile(q0, dt)), lay(tile(qd0, dt))
                zeros = torch.zeros_like(qd)
                for K, targets in SETS.items():
                    poses = corner_poses(K)
                    tg = torch.tensor(targets, device="cuda")
                    offs = torch.tensor(poses[:, 9:], device="cuda", dtype=dt)
                    lin = torch.tensor([6 * k + 3 + i for k in range(K) for i in range(3)], device="cuda")
                    f_ext = torch.zeros((B, n, 6) if aos else (6 * n, B), dtype=dt, device="cuda")
                    W = torch.empty((B, 6 * K, 6 * K) if aos else (36 * K * K, B), dtype=dt, device="cuda")
                    out = (torch.empty_like(qd), torch.empty((B, K, 6) if aos else (6 * K, B), dtype=dt, device="cuda"), torch.empty(B, dtype=dt, device="cuda"))
                    out2 = out[:2]

                    def composed(sweeps):
                        _, _, twist = hm.rnea_bodies(q, qd, qd, ZERO_G, None, layout)
                        X = hm.body_poses(q, targets, poses, layout)
                        hm.apparent_inertia_inverse(q, targets, poses, True, layout, out=W)
                        Wb = W if aos else W.t().reshape(B, 6 * K, 6 * K)
                        tw = (twist if aos else twist.t().reshape(B, n, 6))[:, tg]
                        nk = (X if aos else X.t().reshape(B, K, 12))[:, :, 6:9]  # R^T e_z: the third row of R
                        Wl = Wb.index_select(1, lin).index_select(2, lin)
                        S = torch.tril(Wl) + torch.tril(Wl, -1).transpose(1, 2)
                        b = (tw[:, :, 3:] + torch.cross(tw[:, :, :3], offs.expand(B, K, 3), dim=2)).reshape(B, 3 * K)  # identity rotations: u = v + w x p
                        rho = 1.0 / (torch.diagonal(S, dim1=1, dim2=2).reshape(B, K, 3).sum(dim=2) + EPS)
                        lam = torch.zeros((B, K, 3), dtype=dt, device="cuda")
                        for _ in range(sweeps):
                            for k in range(K):
                                nn = nk[:, k]
                                u = b[:, 3 * k:3 * k + 3] + torch.bmm(S[:, 3 * k:3 * k + 3, :], lam.view(B, 3 * K, 1)).squeeze(2) + EPS * lam[:, k]
                                x = lam[:, k] - rho[:, k, None] * u
                                s = (nn * x).sum(dim=1)
                                t = x - s[:, None] * nn
                                r = t.norm(dim=1)
                                s1 = (s + MU * r) / (1.0 + MU * MU)
                                y = s1[:, None] * nn + (MU * s1 / r)[:, None] * t
                                lam[:, k] = torch.where((r <= MU * s)[:, None], x, torch.where((MU * r <= -s)[:, None], torch.zeros_like(x), y))
                        fb = torch.zeros((B, n, 6), dtype=dt, device="cuda")
                        mom = torch.cross(offs.expand(B, K, 3), lam, dim=2)
                        fb.index_add_(1, tg, torch.cat([mom, lam], dim=2))
                        fl = fb if aos else fb.reshape(B, -1).t().contiguous()
                        return hm.aba(q, zeros, zeros, ZERO_G, fl, layout) + qd

                    def call(sweeps):
                        return hm.contact_impulse(q, qd, targets, [MU] * K, poses, compliance=EPS, iterations=sweeps, layout=layout, out=out)

                    shared = {
                        "  rnea_bodies alone": lambda: hm.rnea_bodies(q, qd, qd, ZERO_G, None, layout),
                        "  apparent COUPLED alone": lambda: hm.apparent_inertia_inverse(q, targets, poses, True, layout, out=W),
                        "  aba with f_ext alone": lambda: hm.aba(q, zeros, zeros, ZERO_G, f_ext, layout),
                        "mh_constraint_impulse (POINT rows; another problem, for scale)":
                            lambda: hm.constraint_impulse(q, qd, targets, [0b111000] * K, poses, compliance=EPS, layout=layout, out=out2),
                    }
                    fast = 20 if B <= 8192 else 3
                    ts = timed(shared, lambda k: fast)
                    say(f"\nB = {B}, {prec}, {lname}, K = {K}")
                    for k, v in ts.items():
                        say(f"  {k:64s} median {np.median(v):10.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    parts = sum(float(np.median(ts[k])) for k in list(shared)[:3])
                    for sweeps in SWEEPS:
                        cands = {"mh_contact_impulse": lambda: call(sweeps), "composition": lambda: composed(sweeps)}
                        ts = timed(cands, lambda k: 1 if k == "composition" else fast)
                        new, old = float(np.median(ts["mh_contact_impulse"])), float(np.median(ts["composition"]))
                        spread = max(ts["mh_contact_impulse"]) - min(ts["mh_contact_impulse"])
                        verdict = "" if new <= old + spread else "   <-- SLOWER than the composition beyond the spread"
                        say(f"  {sweeps:4d} sweeps: mh_contact_impulse {new:10.1f} us (min {min(ts['mh_contact_impulse']):.1f}, max {max(ts['mh_contact_impulse']):.1f}), "
                            f"solve kernel alone {new - parts:10.1f} us, composition {old:12.1f} us, composition / call = {old / new:7.1f}{verdict}")
                    if K <= 4 or dt == torch.float32:  # both forms of the solve are possible: S in LDS against S streamed
                        for path, pname in ((1, "LDS-resident"), (0, "streamed")):
                            _lib.check(lib.mh_internal_contact_path(hm._h, path))
                            ts = timed({"x": lambda: call(200)}, lambda k: fast)
                            say(f"   200 sweeps, {pname:12s} forced: {np.median(ts['x']):10.1f} us (min {min(ts['x']):.1f}, max {max(ts['x']):.1f})")
                        _lib.check(lib.mh_internal_contact_path(hm._h, -1))
                    del f_ext, W, out, out2
                del q, qd, zeros
                torch.cuda.empty_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "contact_dynamics_rates.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
