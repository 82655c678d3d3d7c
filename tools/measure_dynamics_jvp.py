"""Times the forward-mode calls mh_rnea_jvp_*, mh_aba_jvp_* and mh_aba_integrate_jvp_* beside, in the same run, (1) the route to the same
vectors through the matrices -- mh_rnea_derivatives_* / mh_aba_derivatives_* / mh_aba_integrate_derivatives_* followed by the torch einsum
with the directions -- and (2) the matching reverse-mode call mh_rnea_vjp_* / mh_aba_vjp_* / mh_aba_integrate_vjp_*.  arm7 and the
humanoid, fp64 / fp32, AoS and SoA, at B = 4 096 and 262 144.  HIP events on the launch stream around `reps` back-to-back repetitions
after a warm-up, the candidates alternated over five rounds, the median per repetition; at B = 4 096 the repetitions are captured into a
graph once and the replay is timed.  Says per row whether the new call beats the matrix route and how it stands to
its VJP twin (the twin's own spread, max - min over the rounds, beside it).  Writes profiles/dynamics_jvp_rates.txt.
Usage: python tools/measure_dynamics_jvp.py [arm7] [humanoid]"""
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
    wanted = sys.argv[1:] or ["arm7", "humanoid"]
    systems = {"arm7": rt.committedBenchmarkSystems()["arm7"], "humanoid": rt.nextHumanoid(np.random.default_rng(43))}
    g, dt = (0.0, 0.0, -9.81), 0.01
    out = open(os.path.join(ROOT, "profiles", "dynamics_jvp_rates.txt"), "w")

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
        for dtype in (torch.float64, torch.float32):
            prec = "fp64" if dtype == torch.float64 else "fp32"
            for B in (4096, 262144):
                hm.reserve(B)
                tile = lambda x: torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous()
                q, qd, qdd, tau = (tile(x) for x in rt.nextState(np.random.default_rng(1), sys_, 4096))
                d1, d2, d3 = (tile(np.random.default_rng(2 + k).uniform(-1.0, 1.0, (4096, nv))) for k in range(3))
                graphed = B <= 8192
                reps = 20 if graphed else 3
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, vl, al, tl, a1, a2, a3 = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau, d1, d2, d3))
                    dx = torch.cat([a1, a2], dim=1 if aos else 0)
                    o_i = hm.rnea_jvp(ql, vl, al, a1, a2, a3, g, None, layout)
                    o_f = hm.aba_jvp(ql, vl, tl, a1, a2, a3, g, None, layout)
                    o_s = hm.step_jvp(dt, ql, vl, tl, a1, a2, a3, g, None, layout)
                    v_i = hm.rnea_vjp(ql, vl, al, a1, g, None, layout)
                    v_f = hm.aba_vjp(ql, vl, tl, a1, g, None, layout)
                    v_s = hm.step_vjp(dt, ql, vl, tl, a1, a2, g, None, layout)
                    m_i = hm.rnea_derivatives(ql, vl, al, g, None, layout)
                    m_f = hm.aba_derivatives(ql, vl, tl, g, None, layout)
                    m_s = hm.step_derivatives(dt, ql, vl, tl, g, None, layout)
                    H = hm.crba(ql, layout)
                    mv = (lambda D, d, r, c: torch.einsum("bij,bj->bi", D, d)) if aos else (lambda D, d, r, c: torch.einsum("ijb,jb->ib", D.view(r, c, B), d))

                    def mat_inverse():  # (H is taken as given: the route is charged the two derivative matrices only)
                        _, Dq, Dv = hm.rnea_derivatives(ql, vl, al, g, None, layout, out=m_i)
                        return mv(Dq, a1, nv, nv) + mv(Dv, a2, nv, nv) + mv(H, a3, nv, nv)

                    def mat_forward():
                        _, Dq, Dv, Hinv = hm.aba_derivatives(ql, vl, tl, g, None, layout, out=m_f)
                        return mv(Dq, a1, nv, nv) + mv(Dv, a2, nv, nv) + mv(Hinv, a3, nv, nv)

                    def mat_step():
                        _, _, _, A, Bm = hm.step_derivatives(dt, ql, vl, tl, g, None, layout, out=m_s)
                        return mv(A, dx, 2 * nv, 2 * nv) + mv(Bm, a3, 2 * nv, nv)

                    trios = (("rnea_jvp", "matrices: rnea_derivatives + einsum", "twin: rnea_vjp"),
                             ("aba_jvp", "matrices: aba_derivatives + einsum", "twin: aba_vjp"),
                             ("step_jvp", "matrices: step_derivatives + einsum", "twin: step_vjp"))
                    cands = {"rnea_jvp": lambda: hm.rnea_jvp(ql, vl, al, a1, a2, a3, g, None, layout, out=o_i),
                             "matrices: rnea_derivatives + einsum": mat_inverse,
                             "twin: rnea_vjp": lambda: hm.rnea_vjp(ql, vl, al, a1, g, None, layout, out=v_i),
                             "aba_jvp": lambda: hm.aba_jvp(ql, vl, tl, a1, a2, a3, g, None, layout, out=o_f),
                             "matrices: aba_derivatives + einsum": mat_forward,
                             "twin: aba_vjp": lambda: hm.aba_vjp(ql, vl, tl, a1, g, None, layout, out=v_f),
                             "step_jvp": lambda: hm.step_jvp(dt, ql, vl, tl, a1, a2, a3, g, None, layout, out=o_s),
                             "matrices: step_derivatives + einsum": mat_step,
                             "twin: step_vjp": lambda: hm.step_vjp(dt, ql, vl, tl, a1, a2, g, None, layout, out=v_s)}
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    say(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        say(f"  {k:40s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    for new, old, twin in trios:
                        spread = max(times[twin]) - min(times[twin])
                        lost = "" if med[new] < med[old] else "   <-- NOT faster than the matrix route"
                        over = "" if med[new] <= med[twin] + spread else "   <-- beyond its VJP twin plus the twin's spread"
                        say(f"  {new}: matrix route / new = {med[old] / med[new]:.1f}, new / twin = {med[new] / med[twin]:.2f} "
                            f"(twin's spread {spread:.1f} us){lost}{over}")
                    del o_i, o_f, o_s, v_i, v_f, v_s, m_i, m_f, m_s, H
                del q, qd, qdd, tau, d1, d2, d3
                torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
