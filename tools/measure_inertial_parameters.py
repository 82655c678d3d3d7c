"""Times mh_rnea_parameters_* / mh_aba_parameters_* (per-configuration inertial parameters) beside, in the same run on the same device,
(1) the same model's run-time-topology mh_rnea_* / mh_aba_* with fixed parameters (a handle created with MH_DISABLE_SPEC=1: no code
object), and (2), for the inverse dynamics, the only route there was before: mh_regressor_* (first-moment columns) followed by the
batched product with pi.  Humanoid and the 128-body tree, fp64 / fp32, AoS / SoA, B = 4 096 and 262 144.  HIP events on the launch
stream around `reps` back-to-back repetitions after a warm-up, the candidates alternated over five rounds, the median per repetition; at
B = 4 096 the 20 repetitions are captured into a graph once and the replay is timed.  The regressor route is
skipped where its matrix does not fit (B * nv * 10 n entries).
Usage: python tools/measure_inertial_parameters.py [humanoid|tree128 ...] (default: both)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from measure_mass_matrix_inverse import measure  # noqa: E402  (the timing protocol)

REGRESSOR_BYTES_CAP = 24 << 30


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    wanted = sys.argv[1:] or ["humanoid", "tree128"]
    systems = {"humanoid": rt.nextHumanoid(np.random.default_rng(43)), "tree128": rt.committedBenchmarkSystems()["tree128"]}
    print(f"device: {torch.cuda.get_device_name(0)}")
    g = (0.0, 0.0, -9.81)
    for name in wanted:
        sys_ = systems[name]
        desc = sys_.toModelDesc()
        os.environ["MH_DISABLE_SPEC"] = "1"
        hm = HipModel(desc)  # run-time topology for every call of this tool
        del os.environ["MH_DISABLE_SPEC"]
        n, nv = desc.n_joints, desc.nv
        own = hm.inertial_parameters().reshape(-1)
        print(f"\nmodel: {name}, {n} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
        for dtype in (torch.float64, torch.float32):
            prec, size = ("fp64", 8) if dtype == torch.float64 else ("fp32", 4)
            for B in (4096, 262144):
                hm.reserve(B)
                st = rt.nextState(np.random.default_rng(1), sys_, 4096)
                q, qd, qdd, tau = (torch.tensor(x, device="cuda", dtype=dtype).repeat((B + 4095) // 4096, 1)[:B].contiguous() for x in st)
                scale = 1.0 + 0.5 * torch.rand((B, 1), device="cuda", dtype=dtype)  # every robot heavier by its own factor (m and J; c kept)
                pi = torch.tensor(own, device="cuda", dtype=dtype).repeat(B, 1).reshape(B, n, 10)
                pi[:, :, 0] *= scale
                pi[:, :, 4:] *= scale[:, :, None]
                pi = pi.reshape(B, 10 * n).contiguous()
                lin = pi.reshape(B, n, 10).clone()
                lin[:, :, 1:4] *= lin[:, :, 0:1]
                lin = lin.reshape(B, 10 * n).contiguous()
                graphed = B <= 8192
                reps = 20 if graphed else 3
                with_regressor = B * nv * 10 * n * size <= REGRESSOR_BYTES_CAP
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, qdl, qddl, taul, pil = (x if aos else x.t().contiguous() for x in (q, qd, qdd, tau, pi))
                    out = torch.empty_like(qdl)
                    cands = {"rnea_parameters": lambda: hm.rnea_parameters(ql, qdl, qddl, pil, g, None, layout, out=out),
                             "rnea, fixed parameters": lambda: hm.rnea(ql, qdl, qddl, g, layout=layout),
                             "aba_parameters": lambda: hm.aba_parameters(ql, qdl, taul, pil, g, None, layout, out=out),
                             "aba, fixed parameters": lambda: hm.aba(ql, qdl, taul, g, layout=layout)}
                    if with_regressor:
                        if aos:
                            route = lambda: torch.einsum("bij,bj->bi", hm.regressor(ql, qdl, qddl, g, layout, first_moment_columns=True), lin)
                        else:
                            lin_t = lin.t().contiguous()
                            route = lambda: torch.einsum("ijb,jb->ib", hm.regressor(ql, qdl, qddl, g, layout, first_moment_columns=True), lin_t)
                        route()
                        cands["(b) regressor + product with pi (eager)"] = route
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    print(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        print(f"  {k:42s} median {med[k]:10.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    print(f"  rnea_parameters / rnea = {med['rnea_parameters'] / med['rnea, fixed parameters']:.2f}; "
                          f"aba_parameters / aba = {med['aba_parameters'] / med['aba, fixed parameters']:.2f}")
                    if with_regressor:
                        k = "(b) regressor + product with pi (eager)"
                        print(f"  regressor route / rnea_parameters = {med[k] / med['rnea_parameters']:.2f}"
                              f"{'' if med['rnea_parameters'] < med[k] else '   <-- NOT faster than the regressor route'}")
                    else:
                        print(f"  regressor route: not run, Y alone is {B * nv * 10 * n * size / 2 ** 30:.1f} GiB")
                    del out
                del q, qd, qdd, tau, pi, lin
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
