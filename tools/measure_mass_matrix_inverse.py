"""Times mh_mass_matrix_inverse_f64 / _f32 (the full matrix and a list of six columns) beside what the same build needs for the same
result without it: (a) one mh_aba_* call with a unit effort per column (nv calls for the matrix; six for the block of the floating joint,
which is what the calculator mirror issued before), and (b), for orientation only, mh_crba_* followed by torch's batched inverse.
HIP events on the launch stream around `reps` back-to-back repetitions after a warm-up, the candidates alternated over five rounds, the
median per repetition; at batches of up to 8 192 configurations a repetition is shorter than the host needs to issue it, so the 20
repetitions are captured into a graph once and the replay is timed; (b) is always timed eagerly.
Usage: python tools/measure_mass_matrix_inverse.py [humanoid|arm7|tree128 ...] (default: all three)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
ROUNDS = 5


def runner(torch, fn, reps, graphed):
    """A callable that issues `reps` repetitions of fn: back-to-back calls, or one replay of a graph that captured them."""
    run = lambda: [fn() for _ in range(reps)]
    if graphed:
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                run()
        torch.cuda.synchronize()
        run = graph.replay
    for _ in range(2):  # warm-up
        run()
    torch.cuda.synchronize()
    return run


def measure(torch, cands, reps, graphed):
    runs = {k: runner(torch, fn, reps, graphed and not k.startswith("(b)")) for k, fn in cands.items()}
    times = {k: [] for k in cands}
    for _ in range(ROUNDS):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return times


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    wanted = sys.argv[1:] or ["humanoid", "arm7", "tree128"]
    systems = {"humanoid": rt.nextHumanoid(np.random.default_rng(43)), "arm7": rt.committedBenchmarkSystems()["arm7"],
               "tree128": rt.committedBenchmarkSystems()["tree128"]}
    plans = {"humanoid": ((torch.float64, torch.float32), (4096, 262144)), "arm7": ((torch.float64,), (4096, 262144)),
             "tree128": ((torch.float32,), (4096,))}
    print(f"device: {torch.cuda.get_device_name(0)}")
    g0 = (0.0, 0.0, 0.0)
    for name in wanted:
        sys_ = systems[name]
        desc = sys_.toModelDesc()
        hm = HipModel(desc)
        nv = desc.nv
        six = list(range(6)) if name != "arm7" else None  # the floating joint's DoFs on the humanoid; six DoFs of the root's subtree on tree128
        print(f"\nmodel: {name}, {desc.n_joints} joints, nv = {nv}, kernel variant: {hm.kernel_variant}")
        for dtype in plans[name][0]:
            prec, size = ("fp64", 8) if dtype == torch.float64 else ("fp32", 4)
            for B in plans[name][1]:
                hm.reserve(B)
                q = torch.tensor(rt.nextState(np.random.default_rng(1), sys_, 4096)[0], device="cuda", dtype=dtype)
                q = q.repeat((B + 4095) // 4096, 1)[:B].contiguous()
                z = torch.zeros((B, nv), dtype=dtype, device="cuda")
                e = z.clone()
                e[:, 0] = 1.0  # one unit effort: the cost of a column does not depend on which
                graphed = B <= 8192
                reps = 20 if graphed else 3
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    ql, zl, el = (x if aos else x.t().contiguous() for x in (q, z, e))
                    out_full = hm.mass_matrix_inverse(ql, None, layout)
                    cands = {"inverse, full matrix": lambda: hm.mass_matrix_inverse(ql, None, layout, out=out_full),
                             "1 x aba": lambda: hm.aba(ql, zl, el, g0, layout=layout),
                             f"(a) {nv} x aba, unit efforts": lambda: [hm.aba(ql, zl, el, g0, layout=layout) for _ in range(nv)]}
                    if six:
                        out_six = hm.mass_matrix_inverse(ql, six, layout)
                        cands["inverse, 6 columns"] = lambda: hm.mass_matrix_inverse(ql, six, layout, out=out_six)
                        cands["(a) 6 x aba, unit efforts"] = lambda: [hm.aba(ql, zl, el, g0, layout=layout) for _ in range(6)]
                    if aos:
                        try:
                            torch.linalg.inv(hm.crba(ql))
                            cands["(b) crba + torch.linalg.inv (eager)"] = lambda: torch.linalg.inv(hm.crba(ql))
                        except Exception as err:  # no batched inverse in this torch build
                            print(f"  (b) not available: {type(err).__name__}")
                    times = measure(torch, cands, reps, graphed)
                    med = {k: float(np.median(v)) for k, v in times.items()}
                    print(f"\n{name} {prec}, B = {B}, {lname}{', graph replay of 20' if graphed else ''}")
                    for k, v in times.items():
                        bw = ""
                        if k.startswith("inverse"):
                            wb = B * size * nv * (nv if "full" in k else 6)
                            bw = f"  {wb / 1e6:.1f} MB written, {wb / (med[k] * 1e-6) / 1e12:.3f} TB/s = {100 * wb / (med[k] * 1e-6) / HBM_PEAK:.1f} % of 8 TB/s"
                        print(f"  {k:38s} median {med[k]:10.1f} us  (min {min(v):.1f}, max {max(v):.1f}){bw}")
                    for new, old in (("inverse, full matrix", f"(a) {nv} x aba, unit efforts"), ("inverse, 6 columns", "(a) 6 x aba, unit efforts")):
                        if new in med:
                            print(f"  {new}: {med[new] / med['1 x aba']:.2f} x one aba call; (a) / new call = {med[old] / med[new]:.2f}"
                                  f"{'' if med[new] < med[old] else '   <-- NOT faster than (a)'}")
                    del out_full
                del q, z, e
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
