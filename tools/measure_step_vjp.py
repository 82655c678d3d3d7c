"""Times mh_aba_integrate_vjp_* beside (1) the route a user of the parent commit takes for the same vectors -- the matrices of
mh_aba_integrate_derivatives_* followed by the two torch einsum contractions with the cotangents --, (2) the floor mh_aba_vjp_*, and the
two elementwise calls mh_integrate_* and mh_integrate_vjp_*.  Humanoid fp64 / fp32 at B = 4 096, 32 768 and 262 144, AoS and SoA.  HIP
events on the launch stream around `reps` back-to-back repetitions after a warm-up, the candidates alternated over five rounds, the median
per repetition; at B = 4 096 the repetitions are captured into a graph once and the replay is timed.  Reports per
row whether the step call is faster than the parent commit's route and whether it costs no more than mh_aba_vjp_* plus twice
mh_integrate_*.  Writes profiles/step_vjp_rates.txt.
Usage: python tools/measure_step_vjp.py [B ...]"""
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
    sizes = [int(x) for x in sys.argv[1:]] or [4096, 32768, 262144]
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm, nv = HipModel(desc), desc.nv
    g, dt = (0.0, 0.0, -9.81), 1.0e-3
    out = open(os.path.join(ROOT, "profiles", "step_vjp_rates.txt"), "w")

    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"model: humanoid, {desc.n_joints} joints, nv = {nv}, kernel variant: {hm.kernel_variant}, dt = {dt}")
    new, old, floor, fwd, bwd = ("step_vjp (qdd, gq, gqd, gtau)", "parent commit: step_derivatives + 2 einsum", "floor: aba_vjp", "integrate",
                                 "integrate_vjp (gq, gqd, gqdd)")
    for dtype in (torch.float64, torch.float32):
        prec = "fp64" if dtype == torch.float64 else "fp32"
        for B in sizes:
            hm.reserve(B)
            rep = lambda x: torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous()
            q, qd, qdd, tau = (rep(x) for x in rt.nextState(np.random.default_rng(1), sys_, 4096))
            ga, gb = (rep(np.random.default_rng(s).uniform(-1.0, 1.0, (4096, nv))) for s in (2, 3))
            graphed = B <= 8192
            reps = 20 if graphed else 3
            for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                aos = layout == _lib.LAYOUT_AOS
                ql, vl, al, tl, gal, gbl = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau, ga, gb))
                out_s = hm.step_vjp(dt, ql, vl, tl, gal, gbl, g, None, layout)
                out_f = hm.aba_vjp(ql, vl, tl, gal, g, None, layout)
                out_b = hm.integrate_vjp(dt, vl, al, gal, gbl, layout)
                out_i = (torch.empty_like(ql), torch.empty_like(vl))
                mats = hm.step_derivatives(dt, ql, vl, tl, g, None, layout, out=(None, None, None) + tuple(
                    torch.empty(s, dtype=dtype, device="cuda") for s in (((B, 2 * nv, 2 * nv), (B, 2 * nv, nv)) if aos else ((4 * nv * nv, B), (2 * nv * nv, B)))))
                gl = torch.cat([gal, gbl], dim=1 if aos else 0)

                def old_route():
                    _, _, _, A, Bm = hm.step_derivatives(dt, ql, vl, tl, g, None, layout, out=mats)
                    if aos:
                        return torch.einsum("bi,bij->bj", gl, A), torch.einsum("bi,bij->bj", gl, Bm)
                    return torch.einsum("ib,ijb->jb", gl, A.view(2 * nv, 2 * nv, B)), torch.einsum("ib,ijb->jb", gl, Bm.view(2 * nv, nv, B))

                cands = {new: lambda: hm.step_vjp(dt, ql, vl, tl, gal, gbl, g, None, layout, out=out_s),
                         old: old_route,
                         floor: lambda: hm.aba_vjp(ql, vl, tl, gal, g, None, layout, out=out_f),
                         fwd: lambda: hm.integrate(dt, ql, vl, al, layout, out=out_i),
                         bwd: lambda: hm.integrate_vjp(dt, vl, al, gal, gbl, layout, out=out_b)}
                times = measure(torch, cands, reps, graphed)
                med = {k: float(np.median(v)) for k, v in times.items()}
                say(f"\nhumanoid {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                for k, v in times.items():
                    say(f"  {k:45s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                budget = med[floor] + 2.0 * med[fwd]
                say(f"  faster than the parent commit's route: {'met' if med[new] < med[old] else 'MISSED'} (route / new = {med[old] / med[new]:.1f})")
                say(f"  no more than aba_vjp + 2 integrate:    {'met' if med[new] <= budget else 'MISSED'} (new / budget = {med[new] / budget:.2f})")
                del out_s, out_f, out_b, out_i, mats, gl
            del q, qd, qdd, tau, ga, gb
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
