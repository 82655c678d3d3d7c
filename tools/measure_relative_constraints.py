"""Times mh_aba_constrained_between_* and mh_constraint_impulse_between_* on the 30-DoF humanoid with the hands welded to each other and the
feet held as points on the root (K = 3, m = 12; W arrives for n_app = 4 frames), beside the rooted mh_aba_constrained_* /
mh_constraint_impulse_* with the same targets and rows: B = 4096 and 262144, fp64 and fp32, AoS and SoA.  HIP events around `reps`
back-to-back calls after a warm-up, the candidates alternated over five rounds; prints the median per call with its spread and the ratio.
There is no pass mark: the ratio is what the 16 / 9 times larger W, the reduction and the extra climbs cost.

The rooted figures come from the parent commit when a file of them is given (two runs, because two builds cannot share a process):
    python tools/measure_relative_constraints.py --rooted-only FILE [--package DIR] [B ...]    # in / against a checkout of the parent
    python tools/measure_relative_constraints.py --rooted-from FILE [B ...]
Without --rooted-from the rooted calls of this build are timed in the same rounds.  Writes profiles/relative_constraints_rates.txt."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS, BASES, ROWS = [19, 6, 12], [23, -1, -1], [0b111111, 0b111000, 0b111000]
GRAVITY = (0.0, 0.0, -9.81)


def take(args, flag):
    if flag not in args:
        return None
    i = args.index(flag)
    value = args[i + 1]
    del args[i:i + 2]
    return value


def main():
    args = sys.argv[1:]
    rooted_only, rooted_from, package = take(args, "--rooted-only"), take(args, "--rooted-from"), take(args, "--package")
    sys.path.insert(0, package or ROOT)
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in args] or [4096, 262144]
    parent = json.load(open(rooted_from)) if rooted_from else None
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    K = len(TARGETS)
    lines, record = [], {}

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"model: humanoid, {desc.n_joints} joints, nv = {desc.nv}, kernel variant: {hm.kernel_variant}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"targets {TARGETS}, bases {BASES}, rows {[bin(r) for r in ROWS]}: K = {K}, m = 12, n_app = {K + sum(b >= 0 for b in BASES)}")
    say("rooted: the same targets and rows with every base at the root, " + ("measured on the parent commit" if parent else "this build, same rounds"))
    for B in batches:
        hm.reserve(B)
        q0, qd0, _, tau0 = rt.nextState(np.random.default_rng(1), sys_, 4096)
        tile = lambda x, dt: torch.tensor(x, device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous()
        for dt, prec in ((torch.float64, "fp64"), (torch.float32, "fp32")):
            for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                aos = layout == _lib.LAYOUT_AOS
                lay = lambda x: x if aos else x.reshape(B, -1).t().contiguous()
                q, qd, tau = lay(tile(q0, dt)), lay(tile(qd0, dt)), lay(tile(tau0, dt))
                out = (torch.empty_like(tau), torch.empty((B, K, 6) if aos else (6 * K, B), dtype=dt, device="cuda"))
                cands = {}
                if not rooted_only:
                    cands["mh_aba_constrained_between"] = lambda: hm.aba_constrained(q, qd, tau, TARGETS, ROWS, gravity=GRAVITY, layout=layout, out=out,
                                                                                     bases=BASES)
                    cands["mh_constraint_impulse_between"] = lambda: hm.constraint_impulse(q, qd, TARGETS, ROWS, layout=layout, out=out, bases=BASES)
                if not parent:
                    cands["mh_aba_constrained"] = lambda: hm.aba_constrained(q, qd, tau, TARGETS, ROWS, gravity=GRAVITY, layout=layout, out=out)
                    cands["mh_constraint_impulse"] = lambda: hm.constraint_impulse(q, qd, TARGETS, ROWS, layout=layout, out=out)
                reps = 20 if B <= 8192 else 3
                times = {k: [] for k in cands}
                for _ in range(2):
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
                key = f"B={B} {prec} {lname}"
                say(f"\nB = {B}, {prec}, {lname}")
                for k, v in times.items():
                    say(f"  {k:32s} median {float(np.median(v)):10.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                med = {k: float(np.median(v)) for k, v in times.items()}
                record[key] = med
                if parent:
                    for k, v in parent[key].items():
                        say(f"  {k + ' (parent commit)':32s} median {v:10.1f} us")
                    med.update(parent[key])
                if not rooted_only:
                    say(f"  between / rooted: accelerations {med['mh_aba_constrained_between'] / med['mh_aba_constrained']:.2f}, "
                        f"impulse {med['mh_constraint_impulse_between'] / med['mh_constraint_impulse']:.2f}")
                del q, qd, tau, out
                torch.cuda.empty_cache()
    if rooted_only:
        with open(rooted_only, "w") as f:
            json.dump(record, f, indent=1)
        return
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "relative_constraints_rates.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
