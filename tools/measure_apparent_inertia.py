"""Times mh_apparent_inertia_inverse_f64 (both block modes) beside the path it replaces on the same build -- 6 K = 24 mh_aba_bodies_f64
calls with unit wrenches -- and beside one mh_aba_bodies_f64 call, on the 30-DoF humanoid, fp64, targets = joints 6 / 12 / 19 / 23 (both
feet, both hands).  HIP events around `reps` back-to-back calls after a warm-up, the candidates alternated over `rounds` rounds; prints
the median per call, the ratios, and bytes written / time against the 8 TB/s HBM peak DESIGN.md section 6 uses.
Usage: python tools/measure_apparent_inertia.py [B ...] (default 4096 262144)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
TARGETS = [6, 12, 19, 23]


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in sys.argv[1:]] or [4096, 262144]
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    nv, n, K = desc.nv, desc.n_joints, len(TARGETS)
    g0 = (0.0, 0.0, 0.0)
    print(f"model: humanoid, {n} joints, nv = {nv}, targets {TARGETS}, kernel variant: {hm.kernel_variant}")
    print(f"device: {torch.cuda.get_device_name(0)}")
    for B in batches:
        hm.reserve(B)
        q = torch.tensor(rt.nextState(np.random.default_rng(1), sys_, 4096)[0], device="cuda").repeat((B + 4095) // 4096, 1)[:B].contiguous()
        z = torch.zeros((B, nv), dtype=torch.float64, device="cuda")
        f = torch.zeros((B, n, 6), dtype=torch.float64, device="cuda")
        f[:, TARGETS[0], 0] = 1.0  # one unit wrench: the cost of a column does not depend on which
        for layout, name in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
            aos = layout == _lib.LAYOUT_AOS
            ql = q if aos else q.t().contiguous()
            fl = f if aos else f.reshape(B, -1).t().contiguous()
            zl = z if aos else z.t().contiguous()
            out_d = hm.apparent_inertia_inverse(ql, TARGETS, None, False, layout)
            out_c = hm.apparent_inertia_inverse(ql, TARGETS, None, True, layout)
            cands = {
                "apparent DIAGONAL": lambda: hm.apparent_inertia_inverse(ql, TARGETS, None, False, layout, out=out_d),
                "apparent COUPLED": lambda: hm.apparent_inertia_inverse(ql, TARGETS, None, True, layout, out=out_c),
                "1 x aba_bodies": lambda: hm.aba_bodies(ql, zl, zl, g0, fl, layout),
                f"{6 * K} x aba_bodies (the old path)": lambda: [hm.aba_bodies(ql, zl, zl, g0, fl, layout) for _ in range(6 * K)],
            }
            reps = 20 if B <= 8192 else 3
            times = {k: [] for k in cands}
            for _ in range(2):  # warm-up of every shape
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
            print(f"\nB = {B}, {name}, fp64")
            for k, v in times.items():
                bw = ""
                if k.startswith("apparent"):
                    wb = B * 8 * (36 * K * K if "COUPLED" in k else 36 * K)
                    bw = f"  {wb / 1e6:.1f} MB written, {wb / (med[k] * 1e-6) / 1e12:.3f} TB/s = {100 * wb / (med[k] * 1e-6) / HBM_PEAK:.1f} % of 8 TB/s"
                print(f"  {k:34s} median {med[k]:10.1f} us  (min {min(v):.1f}, max {max(v):.1f}){bw}")
            old, one = med[f"{6 * K} x aba_bodies (the old path)"], med["1 x aba_bodies"]
            for k in ("apparent DIAGONAL", "apparent COUPLED"):
                print(f"  {k}: {med[k] / one:.2f} x one aba_bodies call; old path / new call = {old / med[k]:.1f}"
                      f"{'' if med[k] < old else '   <-- NOT faster than the old path'}")
        del q, z, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
