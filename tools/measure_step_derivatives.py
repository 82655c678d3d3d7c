"""Times mh_aba_integrate_derivatives_* beside what a user of the parent commit does for the pair (A, B): mh_aba_derivatives_* plus the
torch assembly of the earlier examples/linearize_humanoid.py (which leaves the transport across the floating joint out and linearises
another update: it is the cost of the old route, not the same matrices).  Humanoid, B = 4 096 and 262 144, fp64 / fp32, AoS / SoA (the
torch assembly takes AoS: in SoA only the one call is timed).  HIP events on the launch stream around `reps` back-to-back repetitions
after a warm-up, the candidates alternated over five rounds, the median per repetition; at B = 4 096 the repetitions are captured into
a graph once and the replay is timed.  Writes profiles/step_derivatives_rates.txt.
Usage: python tools/measure_step_derivatives.py"""
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
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm, nv, dt, g = HipModel(desc), desc.nv, 1.0e-3, (0.0, 0.0, -9.81)
    out = open(os.path.join(ROOT, "profiles", "step_derivatives_rates.txt"), "w")

    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"model: humanoid, {desc.n_joints} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
    for dtype in (torch.float64, torch.float32):
        prec, size = ("fp64", 8) if dtype == torch.float64 else ("fp32", 4)
        for B in (4096, 262144):
            hm.reserve(B)
            base = rt.nextState(np.random.default_rng(1), sys_, 4096)
            q, qd, _, tau = (torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous() for x in base)
            graphed = B <= 8192
            reps = 20 if graphed else 3
            for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                aos = layout == _lib.LAYOUT_AOS
                ql, vl, tl = (x if aos else x.t().contiguous() for x in (q, qd, tau))
                out_s = hm.step_derivatives(dt, ql, vl, tl, g, None, layout)
                out_s = (None, None, None) + out_s[3:]  # the matrices alone, as the old route gives them
                cands = {"step_derivatives (A, B)": lambda: hm.step_derivatives(dt, ql, vl, tl, g, None, layout, out=out_s)}
                if aos:
                    out_f = hm.aba_derivatives(ql, vl, tl, g, None, layout)
                    eye = torch.eye(nv, dtype=dtype, device="cuda").expand(B, -1, -1)
                    zero = torch.zeros((B, nv, nv), dtype=dtype, device="cuda")

                    def old_route():
                        _, dq, dv, Hinv = hm.aba_derivatives(ql, vl, tl, g, None, layout, out=out_f)
                        bottom = torch.cat([dt * dq, eye + dt * dv], dim=2)
                        A = torch.cat([torch.cat([eye, zero], dim=2) + dt * bottom, bottom], dim=1)
                        return A, torch.cat([dt * dt * Hinv, dt * Hinv], dim=1)

                    cands["parent commit: aba_derivatives + torch assembly"] = old_route
                    cands["aba_derivatives alone"] = lambda: hm.aba_derivatives(ql, vl, tl, g, None, layout, out=out_f)
                times = measure(torch, cands, reps, graphed)
                med = {k: float(np.median(v)) for k, v in times.items()}
                say(f"\nhumanoid {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                for k, v in times.items():
                    bw = ""
                    if k.startswith("step"):
                        wb = B * size * 6 * nv * nv
                        bw = f"  {wb / 1e6:.1f} MB of A and B, {wb / (med[k] * 1e-6) / 1e12:.3f} TB/s of stores over the whole call"
                    say(f"  {k:50s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f}){bw}")
                if aos:
                    new, old = med["step_derivatives (A, B)"], med["parent commit: aba_derivatives + torch assembly"]
                    say(f"  parent commit's route / step_derivatives = {old / new:.2f}{'' if new < old else '   <-- NOT faster than the old route'}")
                    say(f"  assembly alone (step_derivatives - aba_derivatives) = {new - med['aba_derivatives alone']:.1f} us")
                del out_s
            del q, qd, tau
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
