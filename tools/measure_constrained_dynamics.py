"""Times mh_aba_constrained_* beside what a caller issues without it for the same result -- mh_aba_bodies, mh_apparent_inertia_inverse
(COUPLED), a torch.linalg Cholesky solve of the selected rows, mh_aba with the wrenches added to f_ext -- in the same session, on the
30-DoF humanoid: feet welded (m = 12) and feet and hands as point contacts (m = 12), fp64 and fp32, AoS and SoA.  Identity target poses, so
that the composition's torch glue is a gather, a solve and a scatter (with poses it would also transform six-vectors; without the root term
of the relative acceleration, which costs it a mh_body_poses call more).  HIP events around `reps` back-to-back calls after a warm-up, the
candidates alternated over five rounds; prints the median per call with its spread, the ratio, and the constraint kernel's share of the
call (the call minus its three reused launches, timed separately in the same rounds).  Also times mh_constraint_impulse_*.
Usage: python tools/measure_constrained_dynamics.py [B ...] (default 4096 262144); writes profiles/constrained_dynamics_rates.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"feet welded": ([6, 12], [0b111111, 0b111111]), "feet and hands as points": ([6, 12, 19, 23], [0b111000] * 4)}
GRAVITY = (0.0, 0.0, -9.81)


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in sys.argv[1:]] or [4096, 262144]
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    nv, n = desc.nv, desc.n_joints
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"model: humanoid, {n} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    for B in batches:
        hm.reserve(B)
        q0, qd0, _, tau0 = rt.nextState(np.random.default_rng(1), sys_, 4096)
        tile = lambda x, dt: torch.tensor(x, device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous()
        for dt, prec in ((torch.float64, "fp64"), (torch.float32, "fp32")):
            for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                aos = layout == _lib.LAYOUT_AOS
                lay = lambda x: x if aos else x.reshape(B, -1).t().contiguous()
                q, qd, tau = lay(tile(q0, dt)), lay(tile(qd0, dt)), lay(tile(tau0, dt))
                for sname, (targets, masks) in SETS.items():
                    K = len(targets)
                    sel = torch.tensor([6 * k + r for k in range(K) for r in range(6) if (masks[k] >> r) & 1], device="cuda")
                    m = int(sel.numel())
                    tg = torch.tensor(targets, device="cuda")
                    f_ext = torch.zeros((B, n, 6) if aos else (6 * n, B), dtype=dt, device="cuda")
                    W = torch.empty((B, 6 * K, 6 * K) if aos else (36 * K * K, B), dtype=dt, device="cuda")
                    out = (torch.empty_like(tau), torch.empty((B, K, 6) if aos else (6 * K, B), dtype=dt, device="cuda"))
                    qdd2 = torch.empty_like(tau)

                    def composed():
                        _, acc, _ = hm.aba_bodies(q, qd, tau, GRAVITY, None, layout)
                        hm.apparent_inertia_inverse(q, targets, None, True, layout, out=W)
                        Wb = W if aos else W.t().reshape(B, 6 * K, 6 * K)
                        ab = acc if aos else acc.t().reshape(B, n, 6)
                        A = Wb.index_select(1, sel).index_select(2, sel)
                        rhs = -ab[:, tg].reshape(B, 6 * K).index_select(1, sel)
                        lam = torch.cholesky_solve(rhs.unsqueeze(2), torch.linalg.cholesky(A)).squeeze(2)
                        full = torch.zeros((B, 6 * K), dtype=dt, device="cuda")
                        full[:, sel] = lam
                        fb = torch.zeros((B, n, 6), dtype=dt, device="cuda")
                        fb[:, tg] = full.view(B, K, 6)
                        fl = fb if aos else fb.reshape(B, -1).t().contiguous()
                        return hm.aba(q, qd, tau, GRAVITY, fl, layout)

                    cands = {
                        "mh_aba_constrained": lambda: hm.aba_constrained(q, qd, tau, targets, masks, gravity=GRAVITY, layout=layout, out=out),
                        "composition": composed,
                        "mh_constraint_impulse": lambda: hm.constraint_impulse(q, qd, targets, masks, layout=layout, out=out),
                        "  aba_bodies alone": lambda: hm.aba_bodies(q, qd, tau, GRAVITY, None, layout),
                        "  apparent COUPLED alone": lambda: hm.apparent_inertia_inverse(q, targets, None, True, layout, out=W),
                        "  aba with f_ext alone": lambda: hm.aba(q, qd, tau, GRAVITY, f_ext, layout),
                    }
                    reps = 20 if B <= 8192 else 3
                    times = {k: [] for k in cands}
                    for _ in range(2):
                        for fn in cands.values():
                            fn()
                    torch.cuda.synchronize()
                    for _ in range(5):
                        for k, fn in cands.items():
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(reps):
                                fn()
                            e1.record()
                            torch.cuda.synchronize()
                            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    say(f"\nB = {B}, {prec}, {lname}, {sname} (K = {K}, m = {m})")
                    for k, v in times.items():
                        say(f"  {k:28s} median {med[k]:10.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    new, old = med["mh_aba_constrained"], med["composition"]
                    spread = max(times["mh_aba_constrained"]) - min(times["mh_aba_constrained"])
                    parts = med["  aba_bodies alone"] + med["  apparent COUPLED alone"] + med["  aba with f_ext alone"]
                    verdict = "" if new <= old + spread else "   <-- SLOWER than the composition beyond the spread"
                    say(f"  composition / single call = {old / new:.2f} (spread of the single call {spread:.1f} us){verdict}")
                    say(f"  constraint kernel: {new - parts:.1f} us = {100 * (new - parts) / new:.0f} % of the call (call minus its reused launches, each timed alone "
                        f"in the call's layout; in AoS the call itself writes W to SoA scratch, cheaper than the AoS W timed alone: a lower bound there)")
                    del f_ext, W, out, qdd2
                del q, qd, tau
                torch.cuda.empty_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "constrained_dynamics_rates.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
