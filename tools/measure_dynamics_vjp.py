"""Times mh_rnea_vjp_* and mh_aba_vjp_* beside (1) the route a user of the parent commit takes for the same gradients -- the matrices of
mh_rnea_derivatives_* / mh_aba_derivatives_* followed by the torch einsum contraction with the cotangent -- and (2) the plain
mh_rnea_* / mh_aba_* call, the floor no gradient can go under.  Humanoid fp64 / fp32 at B = 4 096, 32 768 and 262 144 and the 128-body
tree in fp32 at B = 4 096 (AoS), AoS and SoA otherwise.  HIP events on the launch stream around `reps` back-to-back repetitions after a warm-up, the
candidates alternated over five rounds, the median per repetition; at B = 4 096 the repetitions are captured into a graph once and the
replay is timed.  Writes profiles/dynamics_vjp_rates.txt.
Usage: python tools/measure_dynamics_vjp.py [humanoid] [tree128]"""
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
    wanted = sys.argv[1:] or ["humanoid", "tree128"]
    systems = {"humanoid": rt.nextHumanoid(np.random.default_rng(43)), "tree128": rt.committedBenchmarkSystems()["tree128"]}
    plans = {"humanoid": ((torch.float64, torch.float32), (4096, 32768, 262144)), "tree128": ((torch.float32,), (4096,))}
    g = (0.0, 0.0, -9.81)
    out = open(os.path.join(ROOT, "profiles", "dynamics_vjp_rates.txt"), "w")

    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    for name in wanted:
        sys_ = systems[name]
        desc = sys_.toModelDesc()
        hm, nv = HipModel(desc), desc.nv
        say(f"\nmodel: {name}, {desc.n_joints} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
        for dtype in plans[name][0]:
            prec = "fp64" if dtype == torch.float64 else "fp32"
            for B in plans[name][1]:
                hm.reserve(B)
                base = rt.nextState(np.random.default_rng(1), sys_, 4096)
                q, qd, qdd, tau = (torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous() for x in base)
                u = torch.tensor(np.random.default_rng(2).uniform(-1.0, 1.0, (4096, nv)), device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous()
                graphed = B <= 8192
                reps = 20 if graphed else 3
                # (the tree in AoS only: the parent commit's forward route takes a third of a second per call there, and its SoA product
                # kernel, whose accesses are B elements apart, many times that -- minutes for one median, and nothing rides on it)
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA"))[:1 if name == "tree128" else 2]:
                    aos = layout == _lib.LAYOUT_AOS
                    ql, vl, al, tl, ul = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau, u))
                    out_i = hm.rnea_vjp(ql, vl, al, ul, g, None, layout)
                    out_f = hm.aba_vjp(ql, vl, tl, ul, g, None, layout)
                    mat_i = hm.rnea_derivatives(ql, vl, al, g, None, layout)
                    mat_f = hm.aba_derivatives(ql, vl, tl, g, None, layout)
                    contract = (lambda D: torch.einsum("bi,bij->bj", ul, D)) if aos else (lambda D: torch.einsum("ib,ijb->jb", ul, D.view(nv, nv, B)))

                    def old_inverse():
                        _, dq, dv = hm.rnea_derivatives(ql, vl, al, g, None, layout, out=mat_i)
                        return contract(dq), contract(dv)

                    def old_forward():
                        _, dq, dv, Hinv = hm.aba_derivatives(ql, vl, tl, g, None, layout, out=mat_f)
                        return contract(dq), contract(dv), contract(Hinv)

                    cands = {"rnea_vjp (gq, gqd, gqdd)": lambda: hm.rnea_vjp(ql, vl, al, ul, g, None, layout, out=out_i),
                             "parent commit: rnea_derivatives + einsum": old_inverse,
                             "floor: rnea": lambda: hm.rnea(ql, vl, al, g, None, layout),
                             "aba_vjp (qdd, gq, gqd, gtau)": lambda: hm.aba_vjp(ql, vl, tl, ul, g, None, layout, out=out_f),
                             "parent commit: aba_derivatives + einsum": old_forward,
                             "floor: aba": lambda: hm.aba(ql, vl, tl, g, None, layout)}
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    say(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        say(f"  {k:45s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    for new, old, floor in (("rnea_vjp (gq, gqd, gqdd)", "parent commit: rnea_derivatives + einsum", "floor: rnea"),
                                            ("aba_vjp (qdd, gq, gqd, gtau)", "parent commit: aba_derivatives + einsum", "floor: aba")):
                        lost = "" if med[new] < med[old] else "   <-- NOT faster than the parent commit's route"
                        say(f"  {new.split()[0]}: parent commit's route / new = {med[old] / med[new]:.1f}, new / floor = {med[new] / med[floor]:.2f}{lost}")
                    del out_i, out_f, mat_i, mat_f
                del q, qd, qdd, tau, u
                torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
