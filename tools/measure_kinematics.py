"""Times mh_body_poses_* (every body) and mh_geometric_jacobian_* (the humanoid's two feet and two hands, with and without the convective
term) in fp64 and fp32, AoS and SoA, at B = 4096 and 262144, and the same on the 128-body tree at B = 131072 in fp32 -- beside two
yardsticks taken in the same run: mh_rnea_bodies_* with both per-body outputs (the same outward sweep, 12 values written per body where
the poses write 12) and mh_centroidal_* (a 6 x nv output), and beside one transposition of the Jacobian's bytes (torch's transposed copy).
HIP events around `reps` back-to-back calls after a warm-up, the candidates alternated over 20 rounds; the median per call is reported.
Every candidate and the two yardsticks the expectations are held to (rnea_bodies through the C-ABI, the transposition as a copy) write
into preallocated outputs; HipModel.centroidal allocates its outputs on every call (torch's caching allocator), which the report states.
Writes the report to the file named on the command line (default profiles/kinematics_rates.txt) and prints it.
Usage: python tools/measure_kinematics.py [report path]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 20
HUMANOID_TARGETS = [6, 12, 19, 23]
TREE_TARGETS = [127, 64]


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kinematics_rates.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    report = open(path, "w")

    def say(text=""):
        print(text, flush=True)
        report.write(text + "\n")
        report.flush()

    def median_us(cands, reps):
        times = {k: [] for k in cands}
        for _ in range(2):
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for k, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}

    say(f"device: {torch.cuda.get_device_name(0)}; median of {ROUNDS} rounds of back-to-back calls, HIP events, microseconds per call")
    misses = []
    systems = rt.committedBenchmarkSystems()
    plan = [("humanoid30", rt.nextHumanoid(np.random.default_rng(43)), HUMANOID_TARGETS, [4096, 262144], ["f64", "f32"]),
            ("tree128", systems["tree128"], TREE_TARGETS, [131072], ["f32"])]
    for name, sys_, targets, batches, dtypes in plan:
        desc = sys_.toModelDesc()
        hm = HipModel(desc)
        nv, n, K = desc.nv, desc.n_joints, len(targets)
        say(f"\nmodel {name}: {n} joints, nv = {nv}, targets {targets}, kernel variant {hm.kernel_variant}")
        base = rt.nextState(np.random.default_rng(1), sys_, 4096)
        for B in batches:
            hm.reserve(B)
            for dtype_name in dtypes:
                dt = torch.float64 if dtype_name == "f64" else torch.float32
                q, qd, qdd = (torch.tensor(x, device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous() for x in base[:3])
                soa_J_time = None
                for layout, lname in ((_lib.LAYOUT_SOA, "SoA"), (_lib.LAYOUT_AOS, "AoS")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, qdl, qddl = (x if aos else x.t().contiguous() for x in (q, qd, qdd))
                    P = hm.body_poses(ql, layout=layout)
                    J = hm.geometric_jacobian(ql, targets, layout=layout)
                    Jc = hm.geometric_jacobian(ql, targets, qd=qdl, convective=True, layout=layout)
                    J2 = J.reshape(B, -1) if aos else J
                    J2t = torch.empty((J2.shape[1], J2.shape[0]), dtype=dt, device="cuda")
                    # mh_rnea_bodies_* with outputs allocated once (HipModel.rnea_bodies makes three tensors per call)
                    import ctypes
                    tau_o = torch.empty_like(qdl)
                    acc_o = torch.empty((B, n, 6) if aos else (6 * n, B), dtype=dt, device="cuda")
                    tw_o = torch.empty_like(acc_o)
                    opts = hm._options(layout, stream=torch.cuda.current_stream().cuda_stream)
                    g3 = (ctypes.c_double * 3)(0.0, 0.0, -9.81)
                    rnea_bodies_fn = getattr(_lib.load(), "mh_rnea_bodies_" + dtype_name)

                    def rnea_bodies(ql=ql, qdl=qdl, qddl=qddl, tau_o=tau_o, acc_o=acc_o, tw_o=tw_o, opts=opts):
                        _lib.check(rnea_bodies_fn(hm._h, B, ql.data_ptr(), qdl.data_ptr(), qddl.data_ptr(), g3, None, ctypes.byref(opts), tau_o.data_ptr(),
                                                  acc_o.data_ptr(), tw_o.data_ptr()))
                    cands = {
                        "poses of all bodies": lambda: hm.body_poses(ql, layout=layout, out=P),
                        f"Jacobians of {K} targets": lambda: hm.geometric_jacobian(ql, targets, layout=layout, out=J),
                        f"Jacobians of {K} targets + convective terms": lambda: hm.geometric_jacobian(ql, targets, qd=qdl, convective=True, layout=layout, out=Jc),
                        "yardstick: rnea_bodies, both per-body outputs": rnea_bodies,
                        "yardstick: centroidal A (allocates its output)": lambda: hm.centroidal(ql, layout=layout),
                        "yardstick: centroidal A and b (allocates its outputs)": lambda: hm.centroidal(ql, qdl, layout=layout),
                        "yardstick: one transposition of the Jacobians' bytes": lambda: J2t.copy_(J2.t()),
                    }
                    med = median_us(cands, 10 if B <= 8192 else 2)
                    say(f"\n{name}  B = {B}  {dtype_name}  {lname}")
                    for k, (m, lo, hi) in med.items():
                        extra = ""
                        if k.startswith("Jacobians") or k.startswith("poses"):
                            nbytes = B * (12 * n if k.startswith("poses") else 6 * K * nv + (6 * K if "convective" in k else 0)) * (8 if dtype_name == "f64" else 4)
                            extra = f"  {nbytes / 1e6:9.1f} MB written, {nbytes / (m * 1e-6) / 1e12:.3f} TB/s"
                        say(f"  {k:55s} median {m:10.1f}  (min {lo:.1f}, max {hi:.1f}){extra}")
                    poses, bodies = med["poses of all bodies"][0], med["yardstick: rnea_bodies, both per-body outputs"][0]
                    verdict = "met" if poses <= bodies else "MISSED"
                    say(f"  expectation: poses not slower than rnea_bodies: {poses:.1f} vs {bodies:.1f} us -- {verdict}")
                    if poses > bodies:
                        misses.append(f"{name} B={B} {dtype_name} {lname}: poses {poses:.1f} us > rnea_bodies {bodies:.1f} us")
                    jt = med[f"Jacobians of {K} targets"][0]
                    if not aos:
                        soa_J_time = jt
                    elif B >= 131072:
                        tr = med["yardstick: one transposition of the Jacobians' bytes"][0]
                        verdict = "met" if jt <= soa_J_time + tr else "MISSED"
                        say(f"  expectation: AoS Jacobians within one transposition of the SoA time: {jt:.1f} vs {soa_J_time:.1f} + {tr:.1f} us -- {verdict}")
                        if jt > soa_J_time + tr:
                            misses.append(f"{name} B={B} {dtype_name}: AoS Jacobians {jt:.1f} us > SoA {soa_J_time:.1f} + transposition {tr:.1f} us")
                    del P, J, Jc, J2, J2t, tau_o, acc_o, tw_o
                del q, qd, qdd
                torch.cuda.empty_cache()
    say("\nexpectations missed: " + ("none" if not misses else ""))
    for m in misses:
        say("  " + m)
    report.close()


if __name__ == "__main__":
    main()
