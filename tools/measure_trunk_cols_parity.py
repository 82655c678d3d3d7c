"""Bias-split forward dynamics (mh_zv_kernels.h, the two-stage hand-off) against the tree-split kernels of the SAME code object (MH_ZV=0),
row for row, at the smallest shapes at which the hand-off of the trunk's columns can still go wrong: humanoid, centaur (two sub-trunks),
torso (revolute root, a one-body late limb) and quadruped (the root is the whole trunk, un-staged fold) at B = 1, 63, 64, 65 and 197 (one
lane, a ragged single group, a full group, a second group with one active lane, four groups); mh_aba_f64, mh_rnea_aba_f64 and the
simulation step mh_aba_integrate_f64 (spec_zv_kernel<.., STEP = true>).  Prints the worst scaled difference max|x - x0| / max(1, max|x0|)
per case (the step: the worst of qdd, q_next and qd_next); tests/test_gpu_trunk_columns.py asserts on the same numbers, against four times
what the commit before the trunk's columns became self-signalling reaches here (profiles/trunk_cols_parity.txt).
python tools/measure_trunk_cols_parity.py [shape ...]     (MH_SPEC_DIR=... for the code objects of another build)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

BATCHES = (1, 63, 64, 65, 197)
SHAPES = ("humanoid", "centaur", "torso", "quadruped")
G = (0.3, -0.2, -9.81)
DT = 1e-3


def system_of(name):
    from mecano_amd import random_tools as rt
    return {"humanoid": rt.nextHumanoid, "centaur": rt.nextCentaur, "torso": rt.nextFixedBaseTorso, "quadruped": rt.nextQuadruped}[name](np.random.default_rng(7))


def models_of(desc):
    """(tree-split model, bias-split model at every batch size) of one description; both must run their topology's code object"""
    from mecano_amd.engine import HipModel
    saved = os.environ.get("MH_ZV")
    try:
        os.environ["MH_ZV"] = "0"
        ref = HipModel(desc)
        os.environ["MH_ZV"] = "2"  # the bias split at every batch size (the default takes it while every job's workgroup gets a CU)
        zv = HipModel(desc)
    finally:
        os.environ.pop("MH_ZV", None)
        if saved is not None:
            os.environ["MH_ZV"] = saved
    assert ref.kernel_variant.startswith("topo:") and zv.kernel_variant.startswith("topo:"), (ref.kernel_variant, zv.kernel_variant)
    return ref, zv


def cases(shapes=SHAPES, batches=BATCHES):
    """[(shape, B, call, scaled worst difference, efforts equal bit for bit)]"""
    import torch
    from mecano_amd import random_tools as rt
    out = []
    for name in shapes:
        sys_ = system_of(name)
        ref, zv = models_of(sys_.toModelDesc())
        for B in batches:
            q, qd, qdd, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(B), sys_, B))
            a0 = ref.aba(q, qd, tau, G)
            t0, a0p = ref.rnea_aba(q, qd, qdd, tau, G)
            s0 = ref.step(DT, q, qd, tau, G)
            for _ in range(2):  # back to back: the second launch finds the sentinels the first one wrote back
                a = zv.aba(q, qd, tau, G)
                t, ap = zv.rnea_aba(q, qd, qdd, tau, G)
                s = zv.step(DT, q, qd, tau, G)
            torch.cuda.synchronize()
            zv.check()
            rel = lambda x, x0: float((x - x0).abs().max()) / max(1.0, float(x0.abs().max()))
            out.append((name, B, "aba", rel(a, a0), True))
            out.append((name, B, "rnea_aba", rel(ap, a0p), bool(torch.equal(t, t0))))
            out.append((name, B, "step", max(rel(x, x0) for x, x0 in zip(s, s0)), True))
    return out


if __name__ == "__main__":
    rows = cases(tuple(sys.argv[1:]) or SHAPES)
    for name, B, call, err, same in rows:
        print(f"{name:9s} B={B:5d} {call:9s} worst scaled difference {err:.3e}" + (f"  efforts bit for bit: {same}" if call == "rnea_aba" else ""))
    for name in dict.fromkeys(r[0] for r in rows):
        print("worst of %-9s %.3e" % (name, max(r[3] for r in rows if r[0] == name)))
