"""Times mh_rnea_parameters_state_vjp_* and mh_aba_parameters_state_vjp_* beside the only route the parent commit has to both the state
and the parameter gradients: the PAIR mh_rnea_vjp_* + mh_rnea_parameters_vjp_*, and mh_aba_vjp_* + mh_aba_parameters_vjp_*, which gives
the state gradients only where every row shares the model's parameters -- so every row of pi holds inertial_parameters() here, for all
candidates alike.  Humanoid and arm7, fp64 / fp32, B = 4 096 and 262 144, AoS and SoA.  HIP events on the launch stream around `reps`
back-to-back repetitions after a warm-up, the candidates alternated over five rounds, the median per repetition; at B = 4 096 the
repetitions are captured into a graph once and the replay is timed.  Each pair is in the rotation twice: the
relative difference of its two medians is the run-to-run spread the comparison is held to.
Writes profiles/parameters_state_vjp_rates.txt.
Usage: python tools/measure_parameters_state_vjp.py [humanoid] [arm7]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_mass_matrix_inverse import measure  # noqa: E402  (the same timing protocol)


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    wanted = sys.argv[1:] or ["humanoid", "arm7"]
    systems = {"humanoid": rt.nextHumanoid(np.random.default_rng(43)), "arm7": rt.committedBenchmarkSystems()["arm7"]}
    g = (0.0, 0.0, -9.81)
    out = open(os.path.join(ROOT, "profiles", "parameters_state_vjp_rates.txt"), "w")
    misses = []

    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    for name in wanted:
        sys_ = systems[name]
        desc = sys_.toModelDesc()
        hm, nv, n = HipModel(desc), desc.nv, desc.n_joints
        own = hm.inertial_parameters()
        say(f"\nmodel: {name}, {n} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
        for dtype in (torch.float64, torch.float32):
            prec = "fp64" if dtype == torch.float64 else "fp32"
            for B in (4096, 262144):
                hm.reserve(B)
                tile = lambda x: torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous()
                q, qd, qdd, tau = (tile(x) for x in rt.nextState(np.random.default_rng(1), sys_, 4096))
                u = tile(np.random.default_rng(2).uniform(-1.0, 1.0, (4096, nv)))
                pi = torch.tensor(own.reshape(1, -1), device="cuda", dtype=dtype).expand(B, n * 10).contiguous()  # shared: the pair's premise
                graphed = B <= 8192
                reps = 20 if graphed else 3
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, vl, al, tl, ul, pl = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau, u, pi))
                    new_i = hm.rnea_parameters_state_vjp(ql, vl, al, pl, ul, g, None, layout)
                    new_f = hm.aba_parameters_state_vjp(ql, vl, tl, pl, ul, g, None, layout)
                    old_i = hm.rnea_vjp(ql, vl, al, ul, g, None, layout) + (hm.rnea_parameters_vjp(ql, vl, al, pl, ul, g, layout),)
                    old_f = hm.aba_vjp(ql, vl, tl, ul, g, None, layout) + (hm.aba_parameters_vjp(ql, vl, tl, pl, ul, g, None, layout)[2],)

                    def pair_inverse():
                        hm.rnea_vjp(ql, vl, al, ul, g, None, layout, out=old_i[:3])
                        hm.rnea_parameters_vjp(ql, vl, al, pl, ul, g, layout, out=old_i[3])

                    def pair_forward():  # (qdd, gq, gqd, gtau) from the first call, gpi from the second, whose qdd and gtau go to scratch
                        hm.aba_vjp(ql, vl, tl, ul, g, None, layout, out=old_f[:4])
                        hm.aba_parameters_vjp(ql, vl, tl, pl, ul, g, None, layout, out=(None, None, old_f[4]))

                    inv, fwd = "rnea_parameters_state_vjp (gq, gqd, gqdd, gpi)", "aba_parameters_state_vjp (qdd, gq, gqd, gtau, gpi)"
                    p_i, p_f = "parent commit: rnea_vjp + rnea_parameters_vjp", "parent commit: aba_vjp + aba_parameters_vjp"
                    cands = {inv: lambda: hm.rnea_parameters_state_vjp(ql, vl, al, pl, ul, g, None, layout, out=new_i),
                             p_i: pair_inverse,
                             fwd: lambda: hm.aba_parameters_state_vjp(ql, vl, tl, pl, ul, g, None, layout, out=new_f),
                             p_f: pair_forward,
                             p_i + ", again": pair_inverse,
                             p_f + ", again": pair_forward}
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    say(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        say(f"  {k:58s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    for new, old, form in ((inv, p_i, "inverse"), (fwd, p_f, "forward")):
                        pair = 0.5 * (med[old] + med[old + ", again"])
                        spread = abs(med[old] - med[old + ", again"]) / pair
                        miss = med[new] > pair * (1.0 + spread)
                        if miss:
                            misses.append(f"{name} {prec} B = {B} {lname} {form} form: {med[new]:.1f} us against {pair:.1f} us")
                        say(f"  {form} form: pair / new = {pair / med[new]:.2f}, spread of the pair {100.0 * spread:.1f} %"
                            f"{'   <-- SLOWER than the pair beyond its spread' if miss else ''}")
                    del new_i, new_f, old_i, old_f
                del q, qd, qdd, tau, u, pi
                torch.cuda.empty_cache()
    say(f"\nmisses: {len(misses)}")
    for m in misses:
        say("  " + m)
    out.close()


if __name__ == "__main__":
    main()
