"""Times mh_rnea_derivatives_* and mh_aba_derivatives_* beside what a user of the parent commit does for the same matrices, in the same
run: the 2 nv + 1 mh_rnea_* calls of a central difference (the perturbing mh_integrate_* calls are not counted, which favours the
baseline), respectively 2 nv + 1 mh_aba_* calls plus one mh_mass_matrix_inverse_*.  Beside them mh_gravity_gradient_* and
mh_crba_coriolis_* at the same size: the same output volume per matrix, the store-bound time the neighbours reach.
HIP events on the launch stream around `reps` back-to-back repetitions after a warm-up, the candidates alternated over five rounds, the
median per repetition; at batches of up to 8 192 states the repetitions are captured into a graph once and the replay is timed
(DESIGN.md section 6.3).  Writes profiles/dynamics_derivatives_rates.txt.
Usage: python tools/measure_dynamics_derivatives.py [humanoid|tree128 ...] (default: both)."""
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
    out = open(os.path.join(ROOT, "profiles", "dynamics_derivatives_rates.txt"), "w")

    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    g = (0.0, 0.0, -9.81)
    for name in wanted:
        sys_ = systems[name]
        desc = sys_.toModelDesc()
        hm = HipModel(desc)
        nv = desc.nv
        say(f"\nmodel: {name}, {desc.n_joints} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
        for dtype in plans[name][0]:
            prec, size = ("fp64", 8) if dtype == torch.float64 else ("fp32", 4)
            for B in plans[name][1]:
                hm.reserve(B)
                base = rt.nextState(np.random.default_rng(1), sys_, 4096)
                q, qd, qdd, tau = (torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous() for x in base)
                graphed = B <= 8192
                reps = 20 if graphed else 3
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, vl, al, tl = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau))
                    out_i = hm.rnea_derivatives(ql, vl, al, g, None, layout)
                    out_f = hm.aba_derivatives(ql, vl, tl, g, None, layout)
                    out_g = hm.gravity_gradient(ql, g, None, layout)
                    n_fd = 2 * nv + 1
                    cands = {"rnea_derivatives": lambda: hm.rnea_derivatives(ql, vl, al, g, None, layout, out=out_i),
                             f"baseline: {n_fd} x rnea": lambda: [hm.rnea(ql, vl, al, g, layout=layout) for _ in range(n_fd)],
                             "aba_derivatives": lambda: hm.aba_derivatives(ql, vl, tl, g, None, layout, out=out_f),
                             f"baseline: {n_fd} x aba + inverse": lambda: ([hm.aba(ql, vl, tl, g, layout=layout) for _ in range(n_fd)],
                                                                           hm.mass_matrix_inverse(ql, None, layout, out=out_f[3])),
                             "gravity_gradient (1 matrix)": lambda: hm.gravity_gradient(ql, g, None, layout, out=out_g)}
                    if aos:  # (the Python face of the Coriolis call allocates its outputs and takes AoS)
                        cands["crba_coriolis (2 matrices, eager alloc)"] = lambda: hm.crba_coriolis(ql, vl)
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    say(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        bw = ""
                        mats = {"rnea_derivatives": 2, "aba_derivatives": 3, "gravity_gradient (1 matrix)": 1}.get(k)
                        if mats:
                            wb = B * size * nv * nv * mats
                            bw = f"  {wb / 1e6:.1f} MB of matrices, {wb / (med[k] * 1e-6) / 1e12:.3f} TB/s"
                        say(f"  {k:42s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f}){bw}")
                    for new, old in (("rnea_derivatives", f"baseline: {n_fd} x rnea"), ("aba_derivatives", f"baseline: {n_fd} x aba + inverse")):
                        say(f"  {old} / {new} = {med[old] / med[new]:.2f}{'' if med[new] < med[old] else '   <-- NOT faster than the baseline'}")
                    say(f"  rnea_derivatives per matrix / gravity_gradient = {med['rnea_derivatives'] / 2 / med['gravity_gradient (1 matrix)']:.2f}")
                    del out_i, out_f, out_g
                del q, qd, qdd, tau
                torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
