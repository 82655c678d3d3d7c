"""Times mh_rnea_parameters_vjp_* and mh_aba_parameters_vjp_* beside (1) the route a user of the parent commit takes for the same
gradients -- mh_regressor_* with first-moment columns, the torch einsum contraction with the cotangent and the chain rule to (m, c, J) in
torch; for the forward form mh_aba_parameters_* and mh_mass_matrix_inverse_* times w in front of it -- and (2) the plain
mh_rnea_parameters_* / mh_aba_parameters_* call at the same size.  Humanoid and arm7, fp64 / fp32, B = 4 096 and 262 144, AoS and SoA.
HIP events on the launch stream around `reps` back-to-back repetitions after a warm-up, the candidates alternated over five rounds, the
median per repetition; at B = 4 096 the repetitions are captured into a graph once and the replay is timed.
Writes profiles/parameters_vjp_rates.txt.
Usage: python tools/measure_parameters_vjp.py [humanoid] [arm7]"""
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
    out = open(os.path.join(ROOT, "profiles", "parameters_vjp_rates.txt"), "w")

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
                pi = tile((own[None] * np.random.default_rng(3).uniform(0.8, 1.25, (4096, n, 1))).reshape(4096, -1))  # every body scaled: physical
                graphed = B <= 8192
                reps = 20 if graphed else 3
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, vl, al, tl, ul, pl = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau, u, pi))
                    out_i = hm.rnea_parameters_vjp(ql, vl, al, pl, ul, g, layout)
                    out_f = hm.aba_parameters_vjp(ql, vl, tl, pl, ul, g, None, layout)
                    out_t, out_a = torch.empty_like(vl), torch.empty_like(vl)
                    # the chain rule on [B, n, 10] (AoS) or [n, 10, B] (SoA) views
                    p3 = pl.view(B, n, 10) if aos else pl.view(n, 10, B)
                    m_, c_ = (p3[:, :, 0:1], p3[:, :, 1:4]) if aos else (p3[:, 0:1], p3[:, 1:4])

                    def chain(ghat):
                        g3 = ghat.reshape(B, n, 10) if aos else ghat.reshape(n, 10, B)
                        gm, gh, gJ = (g3[:, :, 0:1], g3[:, :, 1:4], g3[:, :, 4:]) if aos else (g3[:, 0:1], g3[:, 1:4], g3[:, 4:])
                        return torch.cat([gm + (c_ * gh).sum(2 if aos else 1, keepdim=True), m_ * gh, gJ], 2 if aos else 1)

                    def contract(x, Y):
                        return torch.einsum("bi,bij->bj", x, Y) if aos else torch.einsum("ib,ijb->jb", x, Y)

                    def old_inverse(x=ul, acc=al):
                        return chain(contract(x, hm.regressor(ql, vl, acc, g, layout, first_moment_columns=True)))

                    def old_forward():
                        a = hm.aba_parameters(ql, vl, tl, pl, g, None, layout, out=out_a)
                        Hinv = hm.mass_matrix_inverse(ql, None, layout)
                        mu = torch.einsum("bij,bj->bi", Hinv, ul) if aos else torch.einsum("ijb,jb->ib", Hinv.view(nv, nv, B), ul)
                        return -old_inverse(mu.contiguous(), a)

                    cands = {"rnea_parameters_vjp": lambda: hm.rnea_parameters_vjp(ql, vl, al, pl, ul, g, layout, out=out_i),
                             "parent commit: regressor + einsum + chain": old_inverse,
                             "beside: rnea_parameters": lambda: hm.rnea_parameters(ql, vl, al, pl, g, None, layout, out=out_t),
                             "aba_parameters_vjp (qdd, gtau, gpi)": lambda: hm.aba_parameters_vjp(ql, vl, tl, pl, ul, g, None, layout, out=out_f),
                             "parent commit: aba_parameters + Hinv w + regressor route": old_forward,
                             "beside: aba_parameters": lambda: hm.aba_parameters(ql, vl, tl, pl, g, None, layout, out=out_a)}
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    say(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        say(f"  {k:58s} median {med[k]:11.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    inv, fwd = "rnea_parameters_vjp", "aba_parameters_vjp (qdd, gtau, gpi)"
                    old_i, old_f = "parent commit: regressor + einsum + chain", "parent commit: aba_parameters + Hinv w + regressor route"
                    lost = "" if med[inv] < med[old_i] else "   <-- NOT faster than the parent commit's route"
                    twice = "" if med[inv] <= 2.0 * med["beside: rnea_parameters"] else "   <-- more than twice rnea_parameters"
                    say(f"  inverse form: parent commit's route / new = {med[old_i] / med[inv]:.1f}{lost}; new / rnea_parameters = "
                        f"{med[inv] / med['beside: rnea_parameters']:.2f}{twice}")
                    budget = 2.0 * med["beside: aba_parameters"] + med[inv]
                    lost = "" if med[fwd] < med[old_f] else "   <-- NOT faster than the parent commit's route"
                    twice = "" if med[fwd] <= budget else "   <-- more than twice aba_parameters plus the inverse form"
                    say(f"  forward form: parent commit's route / new = {med[old_f] / med[fwd]:.1f}{lost}; new / (2 aba_parameters + inverse form) = "
                        f"{med[fwd] / budget:.2f}{twice}")
                    del out_i, out_f
                del q, qd, qdd, tau, u, pi
                torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
