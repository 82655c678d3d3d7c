"""Stamps of the TAIL of the bias-split forward dynamics (bias fold and outward sweep, per wave and per body; 100 MHz real-time counter);
needs the code object built with -DMH_ZV_PROBE -DMH_ZV_PROBE_TAIL:
EXP_DIR=build/exp_probe python tools/isa.py --so -DMH_ZV_PROBE -DMH_ZV_PROBE_TAIL ; MH_SPEC_DIR=build/exp_probe python tools/exp_zv_tail.py [B]"""
import ctypes, os, sys, glob
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np, torch
from mecano_amd import random_tools as rt
from mecano_amd.engine import HipModel
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
sys_ = rt.nextHumanoid(np.random.default_rng(43))
desc = sys_.toModelDesc()
hm = HipModel(desc)
so = ctypes.CDLL(glob.glob(os.path.join(os.environ["MH_SPEC_DIR"], "libmecano_hip_topo_b5c1*.so"))[0])
q, qd, qdd, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(1), sys_, B))
g = (0, 0, -9.81)
for _ in range(8):
    hm.rnea_aba(q, qd, qdd, tau, g)
    torch.cuda.synchronize()
G = min((B + 63) // 64, 4096)
b = np.zeros(4096 * 3 * 4 * 16, dtype=np.uint64)
assert so.mh_spec_zv_probe_read(b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(b.nbytes)) == 0
st = b.reshape(4096, 3, 4, 16)[:G].astype(np.int64)
bb = np.zeros(4096 * 32 * 4, dtype=np.uint64)
assert so.mh_spec_zv_probe_body_read(bb.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(bb.nbytes)) == 0
bb = bb.reshape(4096, 32, 4)[:G].astype(np.int64)
t0 = st[:, :, :, 15].min()
med = lambda a: np.median(a - t0) / 100
print("B", B, "variant", hm.kernel_variant, "(us after the first entry of the launch; median over the groups)")
names = ["root_in", "taken", "fold_entered", "early_fold", "late_fold+sub", "root_fold", "out", "copied"]
for w in range(4):
    print(f"inertia job wave {w}: " + "  ".join(f"{n}={med(st[:, 1, w, k]):6.2f}" for n, k in zip(names, (4, 5, 6, 7, 8, 9, 10, 11))))
print("taken -> first fold instruction, per wave: " + "  ".join("%.2f" % (np.median(st[:, 1, w, 6] - st[:, 1, w, 5]) / 100) for w in range(4)))
print("last outward instruction -> results copied (kernel end), per wave: " + "  ".join("%.2f" % (np.median(st[:, 1, w, 11] - st[:, 1, w, 10]) / 100) for w in range(4)))
print("slowest wave's last outward instruction -> copied: %.2f us; span of the launch %.2f us" % (np.median(st[:, 1, :, 11].max(axis=1) - st[:, 1, :, 10].max(axis=1)) / 100, (st[:, :2, :, :12].max() - t0) / 100))
parent = np.asarray(desc.parent).astype(int)
print("per body: parent | fold: children_folded  handed_up (step) | outward: entered  acceleration_formed (step)")
for j in range(hm.n_joints):
    m = [med(bb[:, j, k]) for k in range(4)]
    print(f"  body {j:2d} (parent {parent[j]:2d}): fold {m[0]:6.2f} {m[1]:6.2f} ({m[1] - m[0]:.2f}) | out {m[2]:6.2f} {m[3]:6.2f} ({m[3] - m[2]:.2f})")
