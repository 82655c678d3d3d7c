"""Times mh_contact_impulse_between_* beside the rooted mh_contact_impulse_* with the same targets and sweeps, and -- in the same rounds --
mh_constraint_impulse_between_* beside mh_constraint_impulse_* with the same targets, bases and POINT rows: what the relative form costs
on top of the rooted one in the contact solve, against what it costs in the constraint solve, whose launches and in-place reduction of W it
shares.  30-DoF humanoid, 50 sweeps, fp64 and fp32, AoS and SoA:
  (a) K = 4, targets [6, 19, 12, 23] against bases [12, 23, -1, 3] (n_app = 7);
  (b) K = 1, hand on hand (n_app = 2);
  (c) K = 8, four corners of a foot on the other foot and of a hand on the other hand (n_app = 16): 9 755 scratch elements per
      configuration, so a batch that does not fit the device is left out and said so.
HIP events around `reps` back-to-back calls after a warm-up, the four candidates alternated over three rounds; prints the median per call
with its spread and the two ratios.  Yardstick: contact between / rooted should not exceed constraint between / rooted of the same run by
more than 10 % (the run-to-run noise of these launches); a miss is marked.  Where contact_plan keeps S in LDS the call is timed again with
each form of the solve forced: the in-place reduction of W runs inside the solve kernel, at the occupancy its plan allows.
Usage: python tools/measure_contact_between.py [B ...] (default 4096 262144); writes profiles/contact_between_rates.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "(a) K = 4, feet and hands in pairs": ([6, 19, 12, 23], [12, 23, -1, 3]),
    "(b) K = 1, hand on hand": ([19], [23]),
    "(c) K = 8, n_app = 16": ([6] * 4 + [19] * 4, [12] * 4 + [23] * 4),
}
SWEEPS = 50
MU, EPS = 0.5, 1.0e-6
POINT = 0b111000


def corner_poses(K):
    out = np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (K, 1))
    if K == 8:
        for k in range(K):
            out[k, 9:] = (0.1 if k & 1 else -0.1, 0.05 if k & 2 else -0.05, -0.05)
    return out


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in sys.argv[1:]] or [4096, 262144]
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    lib = _lib.load()
    nv, n = desc.nv, desc.n_joints
    lines, misses = [], 0

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def timed(cands, reps, rounds=3):
        times = {k: [] for k in cands}
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
        return times

    say(f"model: humanoid, {n} joints, nv = {nv}, kernel variant: {hm.kernel_variant}; mu = {MU}, compliance = {EPS}, {SWEEPS} sweeps")
    say(f"device: {torch.cuda.get_device_name(0)}")
    free = torch.cuda.mem_get_info()[0]
    for B in batches:
        hm.reserve(B)
        q0, qd0, _, _ = rt.nextState(np.random.default_rng(1), sys_, 4096)
        tile = lambda x, dt: torch.tensor(x, device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous()
        for dt, prec, size in ((torch.float64, "fp64", 8), (torch.float32, "fp32", 4)):
            for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                aos = layout == _lib.LAYOUT_AOS
                lay = lambda x: x if aos else x.reshape(B, -1).t().contiguous()
                q, qd = lay(tile(q0, dt)), lay(tile(qd0, dt))
                for title, (targets, bases) in CASES.items():
                    K = len(targets)
                    n_app = K + sum(b >= 0 for b in bases)
                    need = B * (36 * n_app * n_app + 18 * K + 12 * n + nv) * size
                    if need > 0.5 * free:
                        say(f"\nB = {B}, {prec}, {lname}, {title}: left out -- the scratch of this batch, {need / 2 ** 30:.1f} GiB, against {free / 2 ** 30:.1f} GiB free")
                        continue
                    poses = corner_poses(K)
                    out = (torch.empty_like(qd), torch.empty((B, K, 6) if aos else (6 * K, B), dtype=dt, device="cuda"), torch.empty(B, dtype=dt, device="cuda"))
                    cands = {
                        "mh_contact_impulse_between": lambda: hm.contact_impulse_between(q, qd, targets, bases, [MU] * K, poses, compliance=EPS,
                                                                                         iterations=SWEEPS, layout=layout, out=out),
                        "mh_contact_impulse (rooted)": lambda: hm.contact_impulse(q, qd, targets, [MU] * K, poses, compliance=EPS, iterations=SWEEPS,
                                                                                  layout=layout, out=out),
                        "mh_constraint_impulse_between (POINT rows)": lambda: hm.constraint_impulse(q, qd, targets, [POINT] * K, poses, compliance=EPS,
                                                                                                    layout=layout, out=out[:2], bases=bases),
                        "mh_constraint_impulse (rooted, POINT rows)": lambda: hm.constraint_impulse(q, qd, targets, [POINT] * K, poses, compliance=EPS,
                                                                                                    layout=layout, out=out[:2]),
                    }
                    ts = timed(cands, 20 if B <= 8192 else 3)
                    med = {k: float(np.median(v)) for k, v in ts.items()}
                    say(f"\nB = {B}, {prec}, {lname}, {title} (n_app = {n_app})")
                    for k, v in ts.items():
                        say(f"  {k:46s} median {med[k]:10.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
                    r_contact = med["mh_contact_impulse_between"] / med["mh_contact_impulse (rooted)"]
                    r_constraint = med["mh_constraint_impulse_between (POINT rows)"] / med["mh_constraint_impulse (rooted, POINT rows)"]
                    miss = r_contact > 1.1 * r_constraint
                    misses += miss
                    say(f"  between / rooted: contact {r_contact:.2f}, constraint {r_constraint:.2f}" +
                        ("   <-- MISS: the contact ratio exceeds the constraint ratio by more than 10 %" if miss else ""))
                    if K <= 4 or dt == torch.float32:  # contact_plan takes LDS here: the same call with each form of the solve forced
                        for path, pname in ((1, "LDS-resident"), (0, "streamed")):
                            _lib.check(lib.mh_internal_contact_path(hm._h, path))
                            tp = timed({"x": cands["mh_contact_impulse_between"], "y": cands["mh_contact_impulse (rooted)"]}, 20 if B <= 8192 else 3)
                            say(f"   {pname:12s} forced: between {np.median(tp['x']):10.1f} us, rooted {np.median(tp['y']):10.1f} us, "
                                f"between / rooted {np.median(tp['x']) / np.median(tp['y']):.2f}")
                        _lib.check(lib.mh_internal_contact_path(hm._h, -1))
                    del out
                del q, qd
                torch.cuda.empty_cache()
    say(f"\n{misses} miss(es) of the yardstick")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "contact_between_rates.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
