"""Bias-split forward dynamics (mh_zv_kernels.h) against the tree-split kernels of the SAME code object (MH_ZV=0), row for row:
mh_aba_f64 and mh_rnea_aba_f64 on the humanoid and the centaur at B = 197, 4 096 and 4 097 (ragged last group).  Prints the worst scaled
difference max|a - a0| / max(1, max|a0|) per case; tests/test_gpu_tail_parity.py asserts on the same numbers.
python tools/measure_tail_parity.py [shape ...]     (MH_SPEC_DIR=... for an experiment build's humanoid)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

BATCHES = (197, 4096, 4097)
SHAPES = ("humanoid", "centaur")
G = (0.3, -0.2, -9.81)


def cases(shapes=SHAPES):
    """[(shape, B, call, scaled worst difference, efforts equal bit for bit)]"""
    import torch
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    out = []
    saved = os.environ.get("MH_ZV")
    try:
        for name in shapes:
            sys_ = {"humanoid": rt.nextHumanoid, "centaur": rt.nextCentaur}[name](np.random.default_rng(7))
            d = sys_.toModelDesc()
            os.environ["MH_ZV"] = "0"
            ref = HipModel(d)
            os.environ["MH_ZV"] = "2"  # the bias split at every batch size (the default takes it while every job's workgroup gets a CU)
            zv = HipModel(d)
            assert ref.kernel_variant.startswith("topo:") and zv.kernel_variant.startswith("topo:"), (ref.kernel_variant, zv.kernel_variant)
            for B in BATCHES:
                q, qd, qdd, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(B), sys_, B))
                a0 = ref.aba(q, qd, tau, G)
                t0, a0p = ref.rnea_aba(q, qd, qdd, tau, G)
                for _ in range(2):  # back to back: the second launch finds the flags and sentinels the first one left
                    a = zv.aba(q, qd, tau, G)
                    t, ap = zv.rnea_aba(q, qd, qdd, tau, G)
                torch.cuda.synchronize()
                zv.check()
                scale = max(1.0, float(a0.abs().max()))
                out.append((name, B, "aba", float((a - a0).abs().max()) / scale, True))
                out.append((name, B, "rnea_aba", float((ap - a0p).abs().max()) / scale, bool(torch.equal(t, t0))))
    finally:
        os.environ.pop("MH_ZV", None)
        if saved is not None:
            os.environ["MH_ZV"] = saved
    return out


if __name__ == "__main__":
    rows = cases(tuple(sys.argv[1:]) or SHAPES)
    for name, B, call, err, same in rows:
        print(f"{name:9s} B={B:5d} {call:9s} worst scaled difference {err:.3e}  efforts bit for bit: {same}")
    print("worst over all cases: %.3e" % max(r[3] for r in rows))
