"""Times mh_gravity_gradient_f64 beside mh_crba_f64 (same model, same batch: the same output size and store pattern) and the N + 1
mh_rnea_f64 calls a finite-difference gradient costs, on the 30-DoF humanoid, fp64.  HIP events around `reps` back-to-back calls after a
warm-up, the candidates alternated over `rounds` rounds; prints the median per call, the ratio, and bytes written / time against the
8 TB/s HBM peak DESIGN.md section 6 uses.  Usage: python tools/measure_gravity_gradient.py [B ...] (default 4096 262144)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in sys.argv[1:]] or [4096, 262144]
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    nv = desc.nv
    g = (0.0, 0.0, -9.81)
    print(f"model: humanoid, {desc.n_joints} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
    print(f"device: {torch.cuda.get_device_name(0)}")
    for B in batches:
        hm.reserve(B)
        q = torch.tensor(rt.nextState(np.random.default_rng(1), sys_, 4096)[0], device="cuda").repeat((B + 4095) // 4096, 1)[:B].contiguous()
        z = torch.zeros((B, nv), dtype=torch.float64, device="cuda")
        f = torch.zeros((B, desc.n_joints, 6), dtype=torch.float64, device="cuda")
        f[:, -1, :] = 1.0
        for layout, name in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
            ql = q if layout == _lib.LAYOUT_AOS else q.t().contiguous()
            fl = f if layout == _lib.LAYOUT_AOS else f.reshape(B, -1).t().contiguous()
            zl = z if layout == _lib.LAYOUT_AOS else z.t().contiguous()
            out = hm.gravity_gradient(ql, g, None, layout)
            cands = {
                "gravity_gradient": lambda: hm.gravity_gradient(ql, g, None, layout, out=out),
                "gravity_gradient+f_ext": lambda: hm.gravity_gradient(ql, g, fl, layout, out=out),
                "gravity_gradient grad only": lambda: hm.gravity_gradient(ql, g, None, layout, out=(None, out[1])),
                "crba": lambda: hm.crba(ql, layout),
                f"{nv + 1} x rnea (finite difference)": lambda: [hm.rnea(ql, zl, zl, g, None, layout, False, False) for _ in range(nv + 1)],
            }
            reps = 20 if B <= 8192 else 5
            times = {k: [] for k in cands}
            for _ in range(3):  # warm-up of every shape
                for fn in cands.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(7):
                for k, fn in cands.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
            written = B * (nv * nv + nv) * 8
            print(f"\nB = {B}, {name}, fp64; bytes written per call (grad + tau): {written / 1e6:.2f} MB")
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, v in times.items():
                bw = ""
                if k.startswith("gravity_gradient") or k == "crba":
                    wb = B * nv * nv * 8 + (B * nv * 8 if k in ("gravity_gradient", "gravity_gradient+f_ext") else 0)
                    bw = f"  {wb / (med[k] * 1e-6) / 1e12:.3f} TB/s written = {100 * wb / (med[k] * 1e-6) / HBM_PEAK:.1f} % of 8 TB/s"
                print(f"  {k:36s} median {med[k]:10.1f} us  (min {min(v):.1f}, max {max(v):.1f}){bw}")
            print(f"  ratio gravity_gradient / crba = {med['gravity_gradient'] / med['crba']:.2f};  finite difference / gravity_gradient = "
                  f"{med[f'{nv + 1} x rnea (finite difference)'] / med['gravity_gradient']:.1f}")
        del q, z, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
