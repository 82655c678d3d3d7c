"""Times mh_body_poses_vjp_* and mh_jacobian_transpose_* on the humanoid in fp64 and fp32, AoS and SoA, at B = 4096 and 262144, for the
two feet and two hands (K = 4) and for every body -- each beside the route it replaces, taken in the same run: HipModel.body_poses +
HipModel.geometric_jacobian + an einsum in torch (every body: two Jacobian calls, of 16 targets and of the rest), and beside mh_body_poses_* alone
for the same targets and one transposition of the cotangents' bytes (torch's transposed copy).  HIP events around `reps` back-to-back calls
after a warm-up, the candidates alternated over ROUNDS rounds; the median per call is reported.  The reverse-mode calls and body_poses
write into preallocated outputs; the matrix route allocates what torch's einsum and the (n; f) formation allocate (the caching allocator),
its Jacobians are preallocated.  Expectations stated and judged in the report: the new call is faster than the matrix route in every row,
and within twice mh_body_poses_* (plus, in AoS, the transposition of the cotangents).
Writes the report to the file named on the command line (default profiles/kinematics_vjp_rates.txt) and prints it.
Usage: python tools/measure_kinematics_vjp.py [report path]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 12
HUMANOID_TARGETS = [6, 12, 19, 23]


def main():
    import torch
    from mecano_amd import _lib
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kinematics_vjp_rates.txt")
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
    sys_ = rt.nextHumanoid(np.random.default_rng(43))
    desc = sys_.toModelDesc()
    hm = HipModel(desc)
    nv, n = desc.nv, desc.n_joints
    say(f"model humanoid30: {n} joints, nv = {nv}, targets {HUMANOID_TARGETS} / every body, kernel variant {hm.kernel_variant}")
    base = rt.nextState(np.random.default_rng(1), sys_, 4096)
    rng = np.random.default_rng(2)
    misses = []
    for B in (4096, 262144):
        hm.reserve(B)
        for dtype_name in ("f64", "f32"):
            dt = torch.float64 if dtype_name == "f64" else torch.float32
            q = torch.tensor(base[0], device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1)[:B].contiguous()
            for layout, lname in ((_lib.LAYOUT_SOA, "SoA"), (_lib.LAYOUT_AOS, "AoS")):
                aos = layout == _lib.LAYOUT_AOS
                ql = q if aos else q.t().contiguous()
                for tname, targets in (("feet and hands (K = 4)", HUMANOID_TARGETS), ("every body", None)):
                    K = n if targets is None else len(targets)
                    lists = [list(range(16)), list(range(16, n))] if targets is None else [targets]

                    def cot(per):
                        x = torch.tensor(rng.uniform(-1, 1, (4096, K, per)), device="cuda", dtype=dt).repeat((B + 4095) // 4096, 1, 1)[:B].contiguous()
                        return x if aos else x.reshape(B, -1).t().contiguous()
                    g, w = cot(12), cot(6)
                    gq = torch.empty((B, nv) if aos else (nv, B), dtype=dt, device="cuda")
                    P = hm.body_poses(ql, targets, layout=layout)
                    Js = [hm.geometric_jacobian(ql, t, layout=layout) for t in lists]
                    g2 = g.reshape(B, -1) if aos else g
                    gt = torch.empty((g2.shape[1], g2.shape[0]), dtype=dt, device="cuda")

                    def contract(wr):  # sum_k J_k^T w_k over the lists of at most 16 targets
                        out, k0 = None, 0
                        for t, J in zip(lists, Js):
                            hm.geometric_jacobian(ql, t, layout=layout, out=J)
                            if aos:
                                part = torch.einsum("bkin,bki->bn", J.view(B, len(t), 6, nv), wr[:, k0:k0 + len(t)])
                            else:
                                part = torch.einsum("kinb,kib->nb", J.view(len(t), 6, nv, B), wr.view(K, 6, B)[k0:k0 + len(t)])
                            out, k0 = part if out is None else out + part, k0 + len(t)
                        return out

                    def matrix_vjp():
                        hm.body_poses(ql, targets, layout=layout, out=P)
                        if aos:
                            R, GR = P[..., :9].reshape(B, K, 3, 3), g[..., :9].reshape(B, K, 3, 3)
                            M = R.transpose(-1, -2) @ GR
                            nn = torch.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], dim=-1)
                            f = (R.transpose(-1, -2) @ g[..., 9:, None])[..., 0]
                            return contract(torch.cat([nn, f], dim=-1))
                        R, G = P.view(K, 12, B), g.view(K, 12, B)
                        M = torch.einsum("kaib,kajb->kijb", R[:, :9].reshape(K, 3, 3, B), G[:, :9].reshape(K, 3, 3, B))
                        nn = torch.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], dim=1)
                        f = torch.einsum("kaib,kab->kib", R[:, :9].reshape(K, 3, 3, B), G[:, 9:])
                        return contract(torch.cat([nn, f], dim=1).reshape(6 * K, B))

                    cands = {
                        "body_poses_vjp": lambda: hm.body_poses_vjp(ql, g, targets, layout=layout, out=gq),
                        "replaced: body_poses + geometric_jacobian + einsum": matrix_vjp,
                        "yardstick: body_poses alone": lambda: hm.body_poses(ql, targets, layout=layout, out=P),
                        "yardstick: one transposition of the cotangents' bytes": lambda: gt.copy_(g2.t()),
                    }
                    if targets is not None:
                        cands["jacobian_transpose"] = lambda: hm.jacobian_transpose(ql, w, targets, layout=layout, out=gq)
                        cands["replaced: geometric_jacobian + einsum"] = lambda: contract(w)
                    # the two routes compute the same thing: the largest difference of the results, before anything is timed
                    apart = float((matrix_vjp() - hm.body_poses_vjp(ql, g, targets, layout=layout)).abs().max())
                    med = median_us(cands, 10 if B <= 8192 else 2)
                    say(f"\nhumanoid30  B = {B}  {dtype_name}  {lname}  {tname}   (|matrix route - body_poses_vjp|_inf = {apart:.2e})")
                    for k, (m, lo, hi) in med.items():
                        say(f"  {k:55s} median {m:10.1f}  (min {lo:.1f}, max {hi:.1f})")
                    poses, tr = med["yardstick: body_poses alone"][0], med["yardstick: one transposition of the cotangents' bytes"][0]
                    allowed = 2.0 * poses + (tr if aos else 0.0)
                    row = f"B={B} {dtype_name} {lname} {tname}"
                    for new, old in (("body_poses_vjp", "replaced: body_poses + geometric_jacobian + einsum"), ("jacobian_transpose", "replaced: geometric_jacobian + einsum")):
                        if new not in med:
                            continue
                        t_new, t_old = med[new][0], med[old][0]
                        say(f"  expectation: {new} faster than the matrix route: {t_new:.1f} vs {t_old:.1f} us ({t_old / t_new:.1f} x) -- {'met' if t_new < t_old else 'MISSED'}")
                        if t_new >= t_old:
                            misses.append(f"{row}: {new} {t_new:.1f} us >= matrix route {t_old:.1f} us")
                        say(f"  expectation: {new} within twice body_poses{' plus the transposition' if aos else ''}: {t_new:.1f} vs {allowed:.1f} us -- {'met' if t_new <= allowed else 'MISSED'}")
                        if t_new > allowed:
                            misses.append(f"{row}: {new} {t_new:.1f} us > 2 x body_poses {poses:.1f}{' + transposition %.1f' % tr if aos else ''} us")
                    del g, w, gq, P, Js, gt, g2
                    torch.cuda.empty_cache()
            del q
    say("\nexpectations missed: " + ("none" if not misses else ""))
    for m in misses:
        say("  " + m)
    report.close()


if __name__ == "__main__":
    main()
