"""The launch planners (mecano_amd/csrc/mh_launch_plans.h) under AddressSanitizer + UndefinedBehaviorSanitizer: index arithmetic over the body
records -- the knapsack's tables of n * (budget + 1) entries, the segment table of the tree split, the patches of the record sets -- and
the fixed arrays of the constraint and contact frame lists, indexed with the caller's joints.  A small stand-alone program includes the
header, holds a few descriptions as plain C++ arrays (the stored ones of tests/golden/model_tables_models.json, the humanoid, and the
128-body tree, whose knapsack tables at 80 slots are the largest), runs every planner at the budgets, CU counts, batches and switches of
tests/test_launch_plans_cpu.py and reads every result end to end (hipcc builds it here for the host; nothing touches a device and nothing
is preloaded).  Exit status 0 and an empty stderr is the assertion."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mecano_amd import build as mbuild
from test_model_tables_cpu import model_desc
from test_model_tables_sanitizers import FIELDS, ROOT

MODELS = ("one_fixed", "chain2", "star", "every_kind_permuted", "forest2", "humanoid30", "tree128")

MAIN = r"""
static long touch(const std::vector<int> &v)
{
   long sum = 0;
   for (int x : v)
      sum += x;
   return sum;
}
static const int64_t kBatches[] = {1, 64, 357, 8192, 98304, 196608, 262144, 393216, 1048576};
static const int kCus[] = {1, 3, 256};
static int run(const char *name, const mh_model_desc &d)
{
   Plan P;
   ModelTables t;
   mh_status st = plan_model(&d, P);
   if (st == MH_OK)
      st = compile_model(&d, P, t);
   if (st != MH_OK)
   {
      printf("%s: status %d -- %s\n", name, (int)st, g_err);
      return 1;
   }
   long sum = 0, plans = 0;
   // frame homes: inverse dynamics, forward dynamics, the fused walk; the knapsack and the leaves-upwards rule
   for (int algo = 0; algo < 3; algo++)
      for (int budget : {0, 9, 24, 48, 60, 80, algo == 0 ? t.rnea_stack : (algo == 1 ? t.aba_stack : t.pair_stack)})
         for (int greedy = 0; greedy < 2; greedy++)
         {
            const FramePlan f = dfs_frames(t.meta, t.n, algo, budget, greedy != 0);
            sum += touch(f.meta) + f.lds_slots + f.glb_slots + f.glb_frames, plans++;
         }
   // launch choice and geometry, with the frames of the budget it picks
   for (int cu : kCus)
      for (int64_t B : kBatches)
         for (int place = -1; place <= 2; place++)
            for (int cap : {-1, 48})
               for (int call = 0; call < 7; call++)
               { // (algo, elem, aos, pair) as tests/test_launch_plans_cpu.py: CHOICE_CALLS
                  const Algo algo = call < 4 ? ALGO_RNEA : ALGO_ABA;
                  const size_t elem = call == 6 ? 4 : (call < 4 ? (call < 2 ? 4 : 8) : (call == 4 ? 4 : 8));
                  const bool pair = call == 6, aos = call < 4 && (call & 1);
                  Switches sw;
                  sw.cu_count = cu, sw.dfs_place = place, sw.dfs_budget = cap;
                  const bool win = !pair && dfs_windows(t, algo, elem, aos);
                  const DfsChoice c = dfs_choose(t, sw, algo, elem, B, win, pair);
                  const FramePlan f = dfs_frames(t.meta, t.n, pair ? 2 : (algo == ALGO_RNEA ? 0 : 1), (int)c.budget, false);
                  const DfsGeometry g = dfs_geometry(c, f.lds_slots, f.glb_slots, f.glb_frames, groups_of(B), cu);
                  sum += touch(f.meta) + g.lds + g.per_cu + g.grid + g.gslots + g.mode, plans++;
               }
   // the run-time tree split, its record sets and launch shapes
   const SplitPlan S = split_rt_plan(t.meta, t.n, t.n_slots);
   sum += S.usable + S.n_trunk + S.n_limbs + S.slots + S.est + S.total + touch(S.trunk_list) + touch(S.seg) + touch(S.xl_ofs) + touch(S.xl) + touch(S.patches), plans++;
   if (S.usable)
   {
      int lds_slots[3];
      for (int k = 0; k < 3; k++)
      {
         const SplitRecords R = split_rt_records(S, t.meta, t.n, k);
         lds_slots[k] = R.lds_slots;
         sum += touch(R.meta) + touch(R.xl) + R.lds_slots, plans++;
      }
      for (int cu : kCus)
         for (int64_t B : kBatches)
            for (size_t elem : {(size_t)4, (size_t)8})
               for (Algo algo : {ALGO_RNEA, ALGO_ABA, ALGO_CRBA})
                  for (int pair = 0; pair < 2; pair++)
                  {
                     const SplitShape s = split_rt_shape(S.slots, lds_slots, cu, elem, algo, B, pair != 0);
                     sum += s.k + s.mode + s.grid + (long)s.lds + (long)split_rt_ws_bytes(S.slots, s.grid, elem), plans++;
                  }
   }
   // the lane workspace
   for (int cu : kCus)
      for (int64_t B : kBatches)
         for (long want : {1L, 8L, 64L})
         {
            const Launch L = plan_launch(cu, B);
            const int parts = launch_parts(cu, L, want);
            sum += (long)lane_ws_bytes(t.n_slots, L, parts, 8) + (long)lane_ws_bound(cu, t.n_slots, L, want, 8), plans++;
         }
   // the frames and the scratch of the constrained and the contact dynamics: the lists of tests/test_launch_plans_cpu.py, refused ones too
   const int n = t.n;
   const int lists[][2][MH_MAX_CONSTRAINT_TARGETS + 1] = {
      // K, then the targets; K again, then the bases
      {{1, n - 1}, {1, -1}}, {{1, n - 1}, {1, 0}}, {{4, 6, 19, 12, 23}, {4, 12, 23, -1, 3}},
      {{8, 3, 4, 5, 6, 7, 8, 9, 10}, {8, -1, -1, -1, -1, -1, -1, -1, -1}}, {{8, 3, 4, 5, 6, 7, 8, 9, 10}, {8, 13, 14, 15, 16, 17, 18, 19, 20}},
      {{8, 0, 0, 0, 0, 0, 0, 0, 0}, {8, n - 1, n - 1, n - 1, n - 1, n - 1, n - 1, n - 1, n - 1}},
      {{1, n}, {1, -1}}, {{1, -1}, {1, -1}}, {{1, 0}, {1, n}}, {{1, 0}, {1, -2}}, {{2, 0, 0}, {2, -1, 0}}};
   const double turned[12] = {0, -1, 0, 1, 0, 0, 0, 0, 1, 0.1, -0.2, 0.3}, sheared[12] = {1, 0.5, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
   for (const auto &list : lists)
      for (const double *pose : {(const double *)nullptr, turned, sheared})
      {
         const int K = list[0][0];
         FrameList F{K, K};
         double given[MH_MAX_CONSTRAINT_TARGETS][12];
         for (int k = 0; k < K; k++)
            std::copy_n(pose ? pose : turned, 12, given[k]);
         mh_status refused = MH_OK;
         for (int k = 0; k < K && refused == MH_OK; k++)
            if ((refused = frame_target(t, F, k, list[0][1 + k], list[1][1 + k], pose ? &given[0][0] : nullptr, name, (k & 1) != 0)) == MH_OK)
            { // the joints are accepted: a pose that is no rotation must be refused, as target k of this call, and no other pose may be
               refused = target_frame<double>(&t, F.tgt[k], F.pose[k], F.app_canon[k], name, k);
               char want[96];
               snprintf(want, sizeof want, "%s: target %d: the 3 x 3 part of its pose is not a rotation", name, k);
               if ((refused != MH_OK) != (pose == sheared) || (refused != MH_OK && (refused != MH_ERR_INVALID_ARGUMENT || !strstr(g_err, want))))
               {
                  printf("%s: target %d: pose check gave status %d -- %s\n", name, k, (int)refused, g_err);
                  return 1;
               }
            }
         plans++;
         if (refused != MH_OK)
         {
            sum += (long)refused + (g_err[0] != 0);
            continue;
         }
         frame_list_close(t, F);
         sum += F.K + F.n_app;
         for (int k = 0; k < F.K; k++)
            sum += F.tgt[k] + F.ext[k] + F.base[k] + F.bext[k] + F.bslot[k];
         double poses = 0.0;
         for (int j = 0; j < F.n_app; j++)
         {
            sum += F.app_joints[j];
            for (int r = 0; r < 12; r++)
               poses += F.app_canon[j][r] + (j < F.K ? F.pose[j][r] : 0.0);
         }
         sum += (long)(1.0e3 * poses);
         for (int twists = 0; twists < 2; twists++)
         {
            const ConScratch s = con_scratch(t.n, t.nv, F.K, F.n_app, twists != 0);
            sum += (long)(s.W + s.rhs + s.body + s.wrench + s.zeros + s.zpose + s.twist + s.total);
         }
      }
   printf("%s: status 0 bodies %d split %d plans %ld checksum %ld\n", name, t.n, (int)S.usable, plans, sum);
   return 0;
}
int main()
{
   int bad = 0;
   MODEL_RUNS
   return bad;
}
"""


def _program():
    src = ['#include "mh_launch_plans.h"', "#include <cstdio>"]
    runs = []
    for name in MODELS:
        desc = model_desc(name)
        for field, ctype in FIELDS:
            kind = int if ctype == "int32_t" else float
            values = [kind(v) for v in np.asarray(getattr(desc, field)).reshape(-1)]
            body = ", ".join(repr(v) for v in values)
            # an array of no entries (the fixed joint's index maps) is one the planners must never read: a pointer one past an object
            src.append(f"static const {ctype} {name}_{field}[{max(1, len(values))}] = {{{body}}};" if values else f"static const {ctype} {name}_{field}_none = 0;")
        ptr = {field: (f"{name}_{field}" if np.asarray(getattr(desc, field)).size else f"&{name}_{field}_none + 1") for field, _ in FIELDS}
        src.append(f"static mh_model_desc {name}()\n{{\n   mh_model_desc d;\n   std::memset(&d, 0, sizeof d);\n"
                   f"   d.n_joints = {int(desc.n_joints)}, d.nq = {int(desc.nq)}, d.nv = {int(desc.nv)};\n"
                   + "".join(f"   d.{field} = {ptr[field]};\n" for field, _ in FIELDS) + "   return d;\n}")
        runs.append(f'bad += run("{name}", {name}());')
    return "\n".join(src) + MAIN.replace("MODEL_RUNS", "\n   ".join(runs))


@pytest.mark.timeout(300)
def test_launch_planners_are_clean_under_asan_and_ubsan(tmp_path):
    hipcc = mbuild.hipcc() if (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")) else None
    if hipcc is None:
        pytest.skip("no hipcc")
    src, exe = tmp_path / "plans.hip", tmp_path / "plans"
    src.write_text(_program())
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mecano_amd", "csrc"), str(src), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(MODELS), run.stdout
    for name in MODELS:
        assert any(line.startswith(name + ": status 0 ") for line in lines), run.stdout
    assert any(line.startswith("tree128: status 0 bodies 128 split 1 ") for line in lines), run.stdout
