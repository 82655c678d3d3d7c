"""Times mh_joint_limit_impulse_* beside what a caller issues without it for the same result -- mh_mass_matrix_inverse_* for the listed
columns, then the same projected Gauss-Seidel sweeps and the combination of the columns written in batched torch -- in the same session:
the humanoid's 24 one-DoF joints and the arm's 7, fp64 and fp32, AoS and SoA, at 10 and 50 sweeps.  Limits +-1, margin 0.25, erp 50 on
random states (about three rows in four closed).  HIP events around `reps` back-to-back calls after a warm-up, the candidates alternated
over three rounds; prints the median per call with its spread, the ratio, the split of the call between its two launches (the listed
columns timed alone in the same rounds) and, at L = 22 in fp64, the LDS-resident against the streamed solve.
Usage: python tools/measure_joint_limits.py [B ...] (default 4096 262144); writes profiles/joint_limits_rates.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEPS = (10, 50)
LOWER, UPPER, MARGIN, ERP, EPS = -1.0, 1.0, 0.25, 50.0, 1.0e-6


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    batches = [int(a) for a in sys.argv[1:]] or [4096, 262144]
    lib = _lib.load()
    lines = []

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
                r = reps(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(r):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / r)
        return times

    say(f"device: {torch.cuda.get_device_name(0)}; limits +-1, margin {MARGIN}, erp {ERP}, compliance {EPS}")
    systems = {"humanoid": rt.nextHumanoid(np.random.default_rng(43)), "arm7": rt.committedBenchmarkSystems()["arm7"]}
    for mname, sys_ in systems.items():
        desc = sys_.toModelDesc()
        hm = HipModel(desc)
        one_dof = [j for j in range(desc.n_joints) if int(desc.joint_type[j]) in (0, 1)]
        ofs_v = np.concatenate([[0], np.cumsum([{0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}[int(t)] for t in desc.joint_type])])
        ofs_q = np.concatenate([[0], np.cumsum([{0: 1, 1: 1, 2: 7, 3: 0, 4: 3, 5: 4}[int(t)] for t in desc.joint_type])])
        say(f"\nmodel: {mname}, {desc.n_joints} joints, nv = {desc.nv}, {len(one_dof)} one-DoF joints, kernel variant: {hm.kernel_variant}")
        for B in batches:
            hm.reserve(B)
            q0, qd0, _, _ = rt.nextState(np.random.default_rng(1), sys_, 4096)
            tile = lambda x, dt: torch.tensor(x, device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous()
            for dt, prec in ((torch.float64, "fp64"), (torch.float32, "fp32")):
                for layout, lname in ((_lib.LAYOUT_AOS, "AoS"), (_lib.LAYOUT_SOA, "SoA")):
                    aos = layout == _lib.LAYOUT_AOS
                    lay = lambda x: x if aos else x.reshape(B, -1).t().contiguous()
                    q, qd = lay(tile(q0, dt)), lay(tile(qd0, dt))
                    lists = [one_dof] + ([one_dof[:22]] if mname == "humanoid" and dt == torch.float64 else [])
                    for joints in lists:
                        L, nv = len(joints), desc.nv
                        d = [int(desc.dof_indices[ofs_v[j]]) for j in joints]
                        c = [int(desc.cfg_indices[ofs_q[j]]) for j in joints]
                        dd, cc = torch.tensor(d, device="cuda"), torch.tensor(c, device="cuda")
                        lo, hi = [LOWER] * L, [UPPER] * L
                        Hinv = torch.empty((B, nv, L) if aos else (nv * L, B), dtype=dt, device="cuda")
                        out = (torch.empty_like(qd), torch.empty((B, L) if aos else (L, B), dtype=dt, device="cuda"), torch.empty(B, dtype=dt, device="cuda"))

                        def composed(sweeps):
                            hm.mass_matrix_inverse(q, d, layout, out=Hinv)
                            Hb = Hinv if aos else Hinv.t().reshape(B, nv, L)
                            qa, va = (q if aos else q.t()), (qd if aos else qd.t())
                            angle = qa.index_select(1, cc)
                            gap_lo, gap_hi = angle - LOWER, UPPER - angle
                            low = gap_lo <= gap_hi
                            s = torch.where(low, 1.0, -1.0).to(dt)
                            gap = torch.where(low, gap_lo, gap_hi)
                            closed = gap <= MARGIN
                            b = s * va.index_select(1, dd) + ERP * gap
                            blk = Hb.index_select(1, dd)
                            S = (torch.tril(blk) + torch.tril(blk, -1).transpose(1, 2)) * s[:, :, None] * s[:, None, :]
                            rho = 1.0 / (torch.diagonal(S, dim1=1, dim2=2) + EPS)
                            lam = torch.zeros((B, L), dtype=dt, device="cuda")
                            for _ in range(sweeps):
                                for i in range(L):
                                    u = b[:, i] + (S[:, i, :] * lam).sum(dim=1) + EPS * lam[:, i]
                                    lam[:, i] = torch.where(closed[:, i], torch.clamp_min(lam[:, i] - rho[:, i] * u, 0.0), 0.0)
                            v = va + torch.bmm(Hb, (s * lam).unsqueeze(2)).squeeze(2)
                            return v if aos else v.t().contiguous()

                        def call(sweeps):
                            return hm.joint_limit_impulse(q, qd, joints, lo, hi, MARGIN, ERP, EPS, sweeps, layout=layout, out=out)

                        fast = 20 if B <= 8192 else 3
                        cols = timed({"x": lambda: hm.mass_matrix_inverse(q, d, layout, out=Hinv)}, lambda k: fast)["x"]
                        say(f"\n{mname}, B = {B}, {prec}, {lname}, L = {L}")
                        say(f"  listed columns alone (the call's first launch)      median {np.median(cols):10.1f} us  (min {min(cols):.1f}, max {max(cols):.1f})")
                        for sweeps in SWEEPS:
                            if L == 22:
                                break
                            ts = timed({"call": lambda: call(sweeps), "composition": lambda: composed(sweeps)}, lambda k: 1 if k == "composition" else fast)
                            new, old = float(np.median(ts["call"])), float(np.median(ts["composition"]))
                            spread = max(ts["call"]) - min(ts["call"])
                            verdict = "" if new <= old + spread else "   <-- SLOWER than the composition beyond the spread"
                            say(f"  {sweeps:4d} sweeps: mh_joint_limit_impulse {new:10.1f} us (min {min(ts['call']):.1f}, max {max(ts['call']):.1f}), "
                                f"solve kernel alone {new - float(np.median(cols)):10.1f} us, composition {old:12.1f} us, composition / call = {old / new:7.1f}{verdict}")
                        if L == 22:  # both forms of the solve are possible in fp64: S in LDS (one workgroup per CU) against S streamed
                            for path, pname in ((1, "LDS-resident"), (0, "streamed")):
                                _lib.check(lib.mh_internal_limit_path(hm._h, path))
                                for sweeps in SWEEPS:
                                    ts = timed({"x": lambda: call(sweeps)}, lambda k: fast)["x"]
                                    say(f"  {sweeps:4d} sweeps, {pname:12s} forced: {np.median(ts):10.1f} us (min {min(ts):.1f}, max {max(ts):.1f})")
                            _lib.check(lib.mh_internal_limit_path(hm._h, -1))
                        del Hinv, out
                    del q, qd
                    torch.cuda.empty_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "joint_limits_rates.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
