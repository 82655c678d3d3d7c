// mh_launch_plans.h -- how a model's tables are launched: grids and lane workspaces of the sweep kernels, the homes of the depth-first
// walks' stack frames (dfs_frames) with the launch policy that picks their LDS budget (dfs_choose, dfs_geometry), the run-time tree split
// (split_rt_plan, split_rt_records, split_rt_shape).  Pure host arithmetic on a ModelTables (mh_model_tables.h), the switches of the
// environment and the device's CU count: nothing here calls the HIP runtime, so every plan can be read -- and this code run under
// sanitizers -- on a machine without a device (mh_internal_launch_plan, tests/test_launch_plans_cpu.py,
// tests/test_launch_plans_sanitizers.py).  mh_api.hip keeps the caches, the mutexes, the uploads and the launches.
//
// Included by one translation unit of the library (mh_api.hip) and by stand-alone test programs: everything lives in an unnamed namespace.
#pragma once
#include "mh_model_tables.h"
#include "mh_dfs_kernels.h"
#include "mh_split_kernels.h"
#include "mh_rnea_vjp_kernels.h"
#include "mh_rnea_jvp_kernels.h"

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <vector>

namespace
{
// What the MH_* environment variables set, read once per model by read_switches() (mh_model_create).  The variables read elsewhere or per
// call are not here: MH_CRBA_LPG, MH_SPEC_DIR, MH_AUTO_BUILD, MH_SPEC_SELFCHECK.
struct Switches
{
   int cu_count = 256;    // the device's (mh_model_create); MH_FAKE_CU_COUNT (measurements): shrink every grid so that one workgroup loops over the batch
   int use_spec = 1;        // MH_DISABLE_SPEC=1 in the environment forces the generic kernels (A/B measurements)
   int use_split = -1;      // MH_SPEC_SPLIT = 0 | 1: never / whenever possible use the tree-split kernels (default: small batches)
   int force_io = -1, force_st = -1; // MH_SPEC_IO / MH_SPEC_ST = 0 | 1 override the heuristics (measurements)
   int use_split_rt = -1; // MH_SPLIT_RT = 0 | 1: never / whenever usable (default: small batches)
   int use_transpose = -1; // MH_GENERIC_TRANSPOSE = 0 | 1 overrides the size heuristic
   int use_dfs = 1;       // MH_DFS=0: the sweep kernels of mh_kernels.h serve plain RNEA / ABA calls too (A/B measurements)
   int use_dfs_pair = 1;  // MH_DFS_PAIR=0: mh_rnea_aba_f32 on big batches issues the two depth-first kernels one after the other, as before round 5
   int dfs_place = -1;    // MH_DFS_PLACE = 0 | 1 | 2: force all-LDS / stack in LDS + hand-over global / all global
   bool dfs_place_greedy = false; // MH_DFS_GREEDY=1: the frames' homes from the leaves upwards as in rounds 2-4 (A/B measurements; dfs_frames)
   int dfs_budget = -1;   // MH_DFS_BUDGET: cap of the stack's LDS budget in slots per wave (measurements)
   int dfs_aba64 = 0;     // fp64 forward dynamics on the depth-first kernel too: bushy trees (mh_model_create), or MH_DFS_ABA64=0|1
   int host_chunk = 0; // MH_HOST_CHUNK: configurations per chunk of the host-pointer pipeline (0 = choose)
   int use_rnea_ahead = 1; // MH_RNEA_AHEAD (see rnea_ahead_ok)
   int use_zv = 1;        // MH_ZV=0: never; 1: while every job's workgroup gets a CU of its own (default); 2: whenever the call qualifies
   int use_zv_step = 1;    // MH_ZV_STEP=0: simulation steps never ride in the bias-split / fused forward dynamics (the one-job tree-split kernel integrates instead)
   int use_zvb = 1;       // MH_ZVB=0: never; 1: batches of two or more groups of 64 configurations per CU (default); 2: whenever the call qualifies; MH_ZVB_WHICH = 1 | 2: one of the two launches only (timing)
   int zvb_which = 3;
   int use_zvf = 1;       // MH_ZVF=0: never the fused one-launch form; 1: where the two-launch form would be taken (default); 2: whenever the call qualifies
   int use_zvf_pair = 1;  // MH_ZVF_PAIR=0: the pair call of device-filling batches as two launches (A/B measurements)
   int zv_same_l2 = 0;    // MH_ZV_SAME_L2=1 (experiment, off by default; one-stage hand-off only: the two-stage form of identity index maps is write-through): bias rows and flag of a group whose two jobs prove to sit behind the same L2
                          // stay in that L2 (workgroup-scope stores) -- cache behaviour the memory model does not promise, for no measured gain
   int contact_path = -1; // no variable of the environment: mh_internal_contact_path (tests, measurements) forces the streamed (0) or the LDS-resident (1) contact solve
   int limit_path = -1;   // likewise mh_internal_limit_path: the streamed (0) or the LDS-resident (1) joint-limit solve
   unsigned zv_wait_ticks = 200000000u; // MH_ZV_WAIT_MS: how long an inertia job waits for its bias rows (100 MHz ticks; default 2 s)
};

enum Algo
{
   ALGO_RNEA,
   ALGO_ABA,
   ALGO_CRBA
};

// groups of 64 configurations: one wave, or one workgroup of four waves, each
long groups_of(int64_t B) { return (B + 63) / 64; }

// resident waves per CU the run-time-topology sweep kernels are launched with (plan_launch; the depth-first kernels take what their
// registers allow instead: dfs_choose)
constexpr int kWavesPerCu = 8;

struct Launch
{
   int block, grid;
   long lanes;
};
Launch plan_launch(int cu_count, int64_t B)
{
   Launch L;
   L.block = 64; // one wave per workgroup: a small batch spreads over as many CUs as it has waves
   long waves = (B + 63) / 64;
   long cap = (long)cu_count * kWavesPerCu; // resident waves: the workspace is sized by the grid, not by B
   L.grid = (int)std::max<long>(1, std::min(waves, cap));
   L.lanes = (long)L.grid * L.block;
   return L;
}

// The lane-workspace kernels, small batches: `parts` waves per group of 64 configurations (the grid's y), each with a workspace block of
// its own -- as many as the call wants while they keep one wave per SIMD.  Kernels whose per-body columns are independent (mass matrix,
// Coriolis matrix, centroidal momentum matrix, joint torque regressor, gravity gradient, dynamics derivatives, the gradient with respect
// to the inertial parameters -- mh_params_vjp_kernels.h, in the model's own n_slots per lane --) want min(8, n), each wave
// taking every parts-th body (mh_kernels.h; measured: profiles/r02_regressor_rates.txt, profiles/r02_column_parts.txt); the kernels that
// work through a list want one wave per target or per group of columns.
int launch_parts(int cu_count, const Launch &L, long want)
{
   return (int)std::max<long>(1, std::min<long>(want, (long)cu_count * 4 / L.grid));
}
// ... the workspace of such a launch: `slots` entries per lane on L.grid * parts waves
size_t lane_ws_bytes(long slots, const Launch &L, int parts, size_t elem)
{
   return (size_t)slots * (size_t)L.lanes * (size_t)parts * elem;
}
// ... and its bound over EVERY batch up to the one L was planned for and every want up to max_want (mh_reserve): grid * parts is not
// monotonic in the batch -- a smaller grid may take more parts -- but never exceeds max(grid, min(want * grid, 4 waves per CU))
// (tests/test_launch_plans_cpu.py sweeps it)
size_t lane_ws_bound(int cu_count, long slots, const Launch &L, long max_want, size_t elem)
{
   const long waves = std::max<long>(L.grid, std::min<long>(max_want * L.grid, (long)cu_count * 4));
   return (size_t)slots * (size_t)waves * (size_t)L.block * elem;
}

// ---- reverse-mode gradients of the dynamics (mh_rnea_vjp_kernels.h): that kernel's own slot plan -- the first workspace slot of every
// body, VS_BODY slots each and VS_BRANCH for a body with a child that does not directly follow it; returns the slots per lane
int vjp_slot_plan(const std::vector<int> &meta, int n, std::vector<int> &slot)
{
   slot.assign((size_t)std::max(1, n), 0);
   int slots = 0;
   for (int e = 0; e < n; e++)
   {
      slot[e] = slots;
      slots += (meta[(size_t)e * mh::MI_STRIDE + mh::MI_FLAGS] & mh::MF_STORE_VA) ? mh::VS_BRANCH : mh::VS_BODY;
   }
   return std::max(slots, 1);
}
// ---- forward-mode derivatives of the dynamics (mh_rnea_jvp_kernels.h): the same idea -- JS_BODY slots a body, JS_BRANCH for a body with
// a child that does not directly follow it, which parks v, a, xi, dv and da for that child
int jvp_slot_plan(const std::vector<int> &meta, int n, std::vector<int> &slot)
{
   slot.assign((size_t)std::max(1, n), 0);
   int slots = 0;
   for (int e = 0; e < n; e++)
   {
      slot[e] = slots;
      slots += (meta[(size_t)e * mh::MI_STRIDE + mh::MI_FLAGS] & mh::MF_STORE_VA) ? mh::JS_BRANCH : mh::JS_BODY;
   }
   return std::max(slots, 1);
}

// Depth-first run-time-topology kernels (mh_dfs_kernels.h): homes of the stack frames, where ABA's hand-over lives, grid.
//
// Frame homes.  A frame (non-leaf bodies only) is written when its body is visited and read when the body is popped, plus one
// read-modify-write per child that is not the last: stack traffic is proportional to the number of non-leaf bodies, and most of those
// sit near the leaves.  On an all-global stack the 128-body tree of BASELINE.json's configs[4] moved 5.3x (RNEA) and 17.7x (ABA) its
// algorithmic bytes through HBM at 4.2 / 5.7 TB/s (profiles/r02_config5_dfs_hbm_pmc.json): the kernels were bound by their own
// workspace.  An all-LDS stack needs 37 KB (RNEA) / 100+ KB (ABA) per wave there, i.e. 1-4 waves per CU, and loses more than it saves.
// So LDS is given a BUDGET per wave (what is left of 160 KB at the occupancy the launch wants) and filled from the leaves upwards: a
// frame is placed in LDS if it fits on top of the deepest LDS path below it.  The live frames of a walk are one root-to-leaf path, so
// every path keeps its LDS sum within the budget; the frames that do not fit -- few, near the root -- go to the wave's global block,
// whose offsets count global-homed ancestors only.
//
// meta: the model's body records as they are now (joint source modes set bits in them); algo 0 | 1 | 2: inverse dynamics, forward
// dynamics, the fused walk of both; greedy: Switches::dfs_place_greedy.  FramePlan::meta is the copy of the records a launch reads.
struct FramePlan
{
   int lds_slots = 0, glb_slots = 0, glb_frames = 0;
   std::vector<int> meta;
};
FramePlan dfs_frames(const std::vector<int> &model_meta, int n, int algo, int budget, bool greedy)
{
   std::vector<int> meta = model_meta, frame(n), below(n, 0), lofs(n, 0), gofs(n, 0);
   std::vector<char> home(n, 0);
   auto MI = [&](int e, int k) -> int & { return meta[(size_t)e * mh::MI_STRIDE + k]; };
   for (int e = 0; e < n; e++) // algo 2: the fused RNEA + ABA walk (the forward dynamics' frame + the inverse dynamics' wrench and acceleration)
      frame[e] = algo == 0 ? mh::rnea_frame_slots(MI(e, mh::MI_TYPE), MI(e, mh::MI_NCH))
                           : (algo == 1 ? mh::aba_frame_slots(MI(e, mh::MI_TYPE), MI(e, mh::MI_NCH)) : mh::pair_frame_slots(MI(e, mh::MI_TYPE), MI(e, mh::MI_NCH)));
   // (The inverse dynamics at twelve waves per CU -- 48 slots per lane -- keeps the old placement: it waits on its frames more than it
   // moves them, and the frames next to the leaves are the ones read back right after they were written: 2.92 ms against 3.00 at 1 M
   // configurations, while at eight waves the knapsack wins 2 %: profiles/r05_c5_frame_placement.txt.)
   bool all_fit = true;
   { // rounds 2-4: from the leaves upwards, whatever the frame is worth
      for (int e = n - 1; e >= 0; e--)
      { // engine order is depth-first: children come after their parent
         int need = below[e];
         if (frame[e] > 0 && below[e] + frame[e] <= budget)
            home[e] = 1, need += frame[e];
         else if (frame[e] > 0)
            all_fit = false;
         const int pe = MI(e, mh::MI_PARENT);
         if (pe >= 0)
            below[pe] = std::max(below[pe], need);
      }
   }
   if (!(greedy || (algo == 0 && budget < 64) || all_fit)) // (every frame in LDS already: nothing to choose)
   { // Round 5: by what a frame in LDS SAVES.  A frame is touched 2 (6 + jx) times under a single child, but under k children it is
     // written at the visit, re-read by every later child (v, w / a), read and written by the pop of every child that is not the last
     // (the 27 accumulators of the forward dynamics, the 6 of the inverse dynamics) and read at its own pop: 100 accesses for 47 slots at
     // k = 2, 500 at k = 8, against 16 for 14 under one child.  The budget binds along every root-to-leaf path, so the best set of homes
     // is a knapsack on the tree: best[e][b] = the accesses saved in e's subtree with b slots left for it = max(sum of best[c][b] over
     // the children (e global), worth(e) + sum of best[c][b - frame(e)] (e in LDS)).  128-body tree of configs[4], 80 slots per lane:
     // 5 314 -> 4 680 global slot accesses per configuration in the fused walk (model), 5 144 -> 4 134 for the forward dynamics at 48.
      std::vector<int> worth(n, 0);
      std::vector<int> with_subtree(n, 0); // children that have children of their own: all but the last of them accumulate in the frame
      for (int e = 0; e < n; e++)          // (the leaves are walked behind them and add to the carry: mh_model_tables.h, event_program)
         if (MI(e, mh::MI_PARENT) >= 0 && MI(e, mh::MI_NCH) > 0)
            with_subtree[MI(e, mh::MI_PARENT)]++;
      for (int e = 0; e < n; e++)
      {
         const int k = MI(e, mh::MI_NCH), jx = mh::jx_slots(MI(e, mh::MI_TYPE)), in_frame = std::max(0, with_subtree[e] - 1);
         if (k == 0)
            continue;
         if (algo == 0)
            worth[e] = k == 1 ? 2 * (6 + jx) : (6 + jx + 12) + (k - 1) * 12 + 6 + in_frame * 12 + (6 + jx);
         else
         {
            const int id = algo == 2 ? 6 : 0; // the inverse dynamics' wrench (and acceleration) beside the forward dynamics' slots
            const int acc = 27 + id;
            worth[e] = k == 1 ? 2 * (6 + jx) + 2 * id
                              : (12 + jx + 6 + id) + (k - 1) * (12 + id) + (in_frame > 0 ? acc + (in_frame - 1) * 2 * acc + acc : 0) + (12 + jx);
         }
      }
      const int W = budget + 1;
      std::vector<long> best((size_t)n * W, 0);
      std::vector<char> take((size_t)n * W, 0);
      std::vector<std::vector<int>> kids(n);
      for (int e = 0; e < n; e++)
         if (MI(e, mh::MI_PARENT) >= 0)
            kids[MI(e, mh::MI_PARENT)].push_back(e);
      for (int e = n - 1; e >= 0; e--) // children come after their parent: their rows are complete
         for (int b = 0; b <= budget; b++)
         {
            long out = 0, in = -1;
            for (int c : kids[e])
               out += best[(size_t)c * W + b];
            if (frame[e] > 0 && frame[e] <= b)
            {
               in = worth[e];
               for (int c : kids[e])
                  in += best[(size_t)c * W + b - frame[e]];
            }
            best[(size_t)e * W + b] = std::max(out, in);
            take[(size_t)e * W + b] = in > out;
         }
      std::vector<int> left(n, budget);
      for (int e = 0; e < n; e++)
      {
         const int pe = MI(e, mh::MI_PARENT);
         if (pe >= 0)
            left[e] = left[pe] - (home[pe] ? frame[pe] : 0);
         home[e] = take[(size_t)e * W + left[e]];
      }
   }
   FramePlan plan;
   for (int e = 0; e < n; e++)
   {
      const int pe = MI(e, mh::MI_PARENT);
      if (pe >= 0)
         lofs[e] = lofs[pe] + (home[pe] ? frame[pe] : 0), gofs[e] = gofs[pe] + (home[pe] ? 0 : frame[pe]);
      if (home[e])
         plan.lds_slots = std::max(plan.lds_slots, lofs[e] + frame[e]);
      else if (frame[e] > 0)
         plan.glb_slots = std::max(plan.glb_slots, gofs[e] + frame[e]), plan.glb_frames++;
   }
   auto code = [&](int e) { return home[e] ? (lofs[e] | mh::DFS_LDS) : gofs[e]; };
   for (int e = 0; e < n; e++)
   {
      const int pe = MI(e, mh::MI_PARENT);
      const int pj = pe >= 0 ? mh::jx_slots(MI(pe, mh::MI_TYPE)) : 0;
      if (algo == 0)
      {
         MI(e, mh::MI_DFS_R) = code(e);
         if (pe >= 0)
            MI(e, mh::MI_PFR_R) = code(pe), MI(e, mh::MI_PVA_R) = code(pe) + 6 + pj;
      }
      else
      {
         MI(e, mh::MI_DFS_A) = code(e);
         if (pe >= 0)
            MI(e, mh::MI_PFR_A) = code(pe), MI(e, mh::MI_PV_A) = code(pe) + 12 + pj, MI(e, mh::MI_PACC_A) = code(pe) + 18 + pj;
         if (algo == 2 && pe >= 0)
         { // the inverse dynamics' slots of the parent's frame: behind the forward dynamics' part
            const int pa = mh::aba_frame_slots(MI(pe, mh::MI_TYPE), MI(pe, mh::MI_NCH));
            MI(e, mh::MI_PFR_R) = code(pe) + pa, MI(e, mh::MI_PVA_R) = code(pe) + pa + 6;
         }
      }
   }
   plan.glb_slots = std::max(plan.glb_slots, 6);
   plan.meta = std::move(meta);
   return plan;
}

// Launch policy.  Occupancy first: the grid wants min(resident cap, waves of the batch) waves, spread over the CUs; the LDS a wave may
// use is 160 KB divided by the waves per CU that follow from it (ABA in fp64 holds the whole register file: 4 waves per CU at most).
// Out of that come the row windows (RNEA on AoS matrices), ABA's hand-over if all of it fits (small models at one wave per CU: measured
// 106 vs 116 us on the humanoid at B = 4096), and the rest is the stack's budget.  MH_DFS_PLACE = 0 | 1 | 2 forces an all-LDS stack
// with the hand-over in LDS / an all-LDS stack / an all-global stack (measurements, tests); MH_DFS_BUDGET=<slots> the budget itself.
struct DfsChoice
{
   long per_cu, budget, hand, b_win, slot_bytes;
   bool hand_lds, occ3;
};
// reads of the switches: cu_count, dfs_place, dfs_budget
DfsChoice dfs_choose(const ModelTables &model, const Switches &sw, Algo algo, size_t elem, int64_t B, bool win, bool pair = false)
{
   DfsChoice c{};
   const long waves = groups_of(B);
   c.b_win = win ? 3L * mh::ROW_WIN * mh::ROW_PITCH * (long)elem : 0;
   c.slot_bytes = 64 * (long)elem;
   const long cus = sw.cu_count;
   // resident waves per CU the kernel's registers allow (hipcc -Rpass-analysis=kernel-resource-usage, round 5): fp32 inverse dynamics on
   // SoA / transposed rows 134-136 VGPRs = three waves per SIMD (with the LDS windows of AoS rows 232-234: two); fp32 forward dynamics
   // 181-184 = two, or 168 in the OCC3 build (48 bytes of scratch) = three, taken beyond eight waves per CU, the fused pair walk 216-219 = two; fp64
   // 254-256 = one.  The grid used to be sized for eight everywhere: an inverse dynamics that could keep twelve waves per CU resident ran
   // with eight (1.88 against 1.56 ms at 524 288 configurations of the 128-body tree, profiles/r05_c5_occ.txt), and a fp64 walk planned
   // its LDS for eight waves of which four were resident.
   // Twelve resident waves per CU finish a round 1.32 x later than eight (measured: 13 % more throughput for 50 % more waves), and the
   // waves loop over the groups of 64 configurations: twelve are taken where they save enough ROUNDS to pay for that -- 196 608 (one round
   // of twelve instead of two of eight) and from 393 216 configurations upwards, not at 262 144 (two rounds either way: 2.05 against 1.9 ms)
   long reg_cap = elem == 8 ? 4 : 8;
   const long wpc = (waves + cus - 1) / cus;
   const bool twelve_pays = ((wpc + 11) / 12) * 132 < ((wpc + 7) / 8) * 100;
   if (elem == 4 && algo == ALGO_RNEA && !win && twelve_pays)
      reg_cap = 12;
   if (elem == 4 && algo == ALGO_ABA && !pair && twelve_pays)
      reg_cap = 12, c.occ3 = true; // the build with a register budget for three waves per SIMD (mh_dfs_kernels.h: OCC3)
   c.per_cu = std::max<long>(1, std::min<long>(reg_cap, (waves + cus - 1) / cus));
   const long full_stack = pair ? model.pair_stack : (algo == ALGO_RNEA ? model.rnea_stack : model.aba_stack);
   c.hand = algo == ALGO_RNEA ? 0 : model.aba_hand;
   if (sw.dfs_place >= 0)
   { // forced placements: give the stack what it needs and let the occupancy follow
      c.budget = sw.dfs_place == 2 ? 0 : full_stack;
      c.hand_lds = sw.dfs_place == 0 && algo == ALGO_ABA && (full_stack + c.hand) * c.slot_bytes + c.b_win <= 160 * 1024;
      if (c.budget * c.slot_bytes + c.b_win > 160 * 1024)
         c.budget = (160 * 1024 - c.b_win) / c.slot_bytes;
   }
   else
   {
      // (a wave's share of the 160 KB, rounded DOWN to 2 KB: LDS is allocated in blocks, and a share that fills 160 KB / per_cu to the byte
      // left room for per_cu - 1 workgroups only -- 98 304 configurations of the 128-body tree, six waves per CU wanted, five resident: 0.99 ms
      // against 0.61 with eight slots less, profiles/r05_c5_rnea_budget.txt)
      const long avail = (160 * 1024 / c.per_cu) / 2048 * 2048 - c.b_win;
      c.hand_lds = algo == ALGO_ABA && (full_stack + c.hand) * c.slot_bytes <= avail;
      c.budget = std::max<long>(0, std::min<long>(full_stack, (avail - (c.hand_lds ? c.hand * c.slot_bytes : 0)) / c.slot_bytes));
      if (sw.dfs_budget >= 0)
         c.budget = std::min<long>(sw.dfs_budget, c.budget);
   }
   return c;
}
bool dfs_windows(const ModelTables &model, Algo algo, size_t elem, bool aos)
{ // AoS matrices with identity index maps and rows that span many cache lines: RNEA reads them through LDS windows (mh_dfs_kernels.h)
   return algo == ALGO_RNEA && aos && model.ident_maps && (long)model.nv * (long)elem >= 512;
}
// What a depth-first launch of `waves` groups takes once the choice's frame plan is known: dynamic LDS bytes, the waves per CU that
// leaves room for, the grid, the slots per lane of a wave's global block, and the kernel build (0: every frame in LDS, 1: every frame
// global -- builds without the per-group branch --, 2: both)
struct DfsGeometry
{
   long lds, per_cu, gslots;
   int grid, mode;
};
DfsGeometry dfs_geometry(const DfsChoice &ch, int lds_slots, int glb_slots, int glb_frames, long waves, long cus)
{
   DfsGeometry g{};
   g.per_cu = ch.per_cu;
   g.lds = (lds_slots + (ch.hand_lds ? ch.hand : 0)) * ch.slot_bytes + ch.b_win;
   if (g.lds > 0)
      g.per_cu = std::max<long>(1, std::min<long>(g.per_cu, (160 * 1024) / g.lds));
   g.grid = (int)std::max<long>(1, std::min(waves, cus * g.per_cu));
   g.gslots = (ch.hand_lds ? 0 : ch.hand) + glb_slots;
   g.mode = glb_frames == 0 ? 0 : (lds_slots == 0 ? 1 : 2);
   return g;
}

// ---- run-time tree split (mh_split_kernels.h): trunk / limbs / owners from the tree alone, made once per model.
// Greedy: the limbs start as the trees of the forest; the largest limb is split at its first branching (the chain down to it joins the
// trunk, the branches become limbs) as long as that shortens the estimated critical path  (trunk bodies) + (bodies of the busiest wave).
struct SplitPlan
{
   bool usable = false;
   int n_trunk = 0, n_limbs = 0, slots = 0, est = 0, total = 0;
   int n_seg[mh::SPLIT_WAVES] = {};
   std::vector<int> trunk_list, seg, xl_ofs; // trunk bodies; per wave its limbs as [first, end) body ranges; per trunk body its range of xl
   std::vector<int> xl;                      // exchange slots of the limbs attached to the trunk bodies (plain slot numbers)
   std::vector<int> patches;                 // (body, field, value) patches of the adapted records
};
SplitPlan split_rt_plan(const std::vector<int> &meta, int n, int n_slots)
{
   SplitPlan S;
   const int W = mh::SPLIT_WAVES;
   auto MI = [&](int e, int k) { return meta[(size_t)e * mh::MI_STRIDE + k]; };
   std::vector<std::vector<int>> ch(n);
   std::vector<int> sz(n, 1), cnt(n, 1), roots; // sz: cost of the subtree in tenths of a 1-DoF body step; cnt: bodies in it
   for (int e = 0; e < n; e++)
   { // measured on the sweep kernels: a 6-DoF joint (LDL^T solve, general transforms) costs about 2.5 revolute steps, a 3-DoF joint 2
      const int t = MI(e, mh::MI_TYPE);
      sz[e] = t == MH_JOINT_SIXDOF ? 25 : ((t == MH_JOINT_PLANAR || t == MH_JOINT_SPHERICAL) ? 20 : (t == MH_JOINT_FIXED ? 4 : 10));
   }
   const std::vector<int> own = sz;
   for (int e = n - 1; e >= 0; e--)
   {
      const int pe = MI(e, mh::MI_PARENT);
      if (pe >= 0)
         sz[pe] += sz[e], cnt[pe] += cnt[e];
   }
   for (int e = 0; e < n; e++)
   {
      const int pe = MI(e, mh::MI_PARENT);
      (pe >= 0 ? ch[pe] : roots).push_back(e);
   }
   const int trunk_weight = 2; // in half bodies; measured in round 2 (DESIGN_HISTORY.md, run-time tree split): 1..3 tie, 4+ splits too little
   std::vector<char> trunk(n, 0);
   std::vector<int> limbs = roots;
   auto estimate = [&](const std::vector<int> &L, int nt, std::vector<int> *owner) {
      std::vector<int> order(L.size());
      for (size_t i = 0; i < L.size(); i++)
         order[i] = (int)i;
      std::sort(order.begin(), order.end(), [&](int a, int b) { return sz[L[a]] != sz[L[b]] ? sz[L[a]] > sz[L[b]] : L[a] < L[b]; });
      int load[mh::SPLIT_WAVES] = {}, cnt[mh::SPLIT_WAVES] = {};
      if (owner)
         owner->assign(L.size(), 0);
      for (int i : order)
      {
         int w = 0;
         for (int k = 1; k < W; k++)
            if (load[k] < load[w])
               w = k;
         load[w] += sz[L[i]], cnt[w]++;
         if (owner)
            (*owner)[i] = w;
      }
      int mx = 0, mc = 0;
      for (int k = 0; k < W; k++)
         mx = std::max(mx, load[k]), mc = std::max(mc, cnt[k]);
      return mc > mh::SPLIT_MAX_SEG ? 1 << 30 : (trunk_weight * nt + 1) / 2 + mx; // a trunk body: light outward steps on every wave + its fold on one while three wait
   };
   int best = estimate(limbs, 0, nullptr), nt = 0, ntc = 0; // trunk cost / trunk bodies
   std::vector<int> best_limbs = limbs;
   std::vector<char> best_trunk = trunk;
   int best_nt = 0, best_ntc = 0;
   for (int iter = 0; iter < n; iter++)
   {
      int big = -1;
      for (size_t i = 0; i < limbs.size(); i++)
         if (big < 0 || sz[limbs[i]] > sz[limbs[big]])
            big = (int)i;
      if (big < 0)
         break;
      int r = limbs[big];
      while (ch[r].size() == 1)
         r = ch[r][0];
      if (ch[r].empty())
         break; // the largest limb is a chain: it cannot be split
      for (int b = limbs[big];; b = ch[b][0])
      {
         trunk[b] = 1, nt += own[b], ntc++;
         if (b == r)
            break;
      }
      limbs.erase(limbs.begin() + big);
      for (int c : ch[r])
         limbs.push_back(c);
      const int est = estimate(limbs, nt, nullptr);
      if (est < best)
         best = est, best_limbs = limbs, best_trunk = trunk, best_nt = nt, best_ntc = ntc;
   }
   int sz_total = 0;
   for (int r0 : roots)
      sz_total += sz[r0];
   S.usable = false;
   if (best_limbs.size() < 2 || best > (3 * sz_total) / 4)
      return S; // a chain, or nothing to gain
   limbs = best_limbs, trunk = best_trunk;
   std::vector<int> owner;
   S.est = estimate(limbs, best_nt, &owner);
   // per wave: limbs in ascending order; exchange records behind the sweep kernels' slots
   std::vector<int> seg((size_t)W * mh::SPLIT_MAX_SEG * 2, 0), xslot(n, -1), trunk_list;
   for (int k = 0; k < W; k++)
      S.n_seg[k] = 0;
   std::vector<int> by_start(limbs.size());
   for (size_t i = 0; i < limbs.size(); i++)
      by_start[i] = (int)i;
   std::sort(by_start.begin(), by_start.end(), [&](int a, int b) { return limbs[a] < limbs[b]; });
   int slots = n_slots;
   for (int i : by_start)
   {
      const int w = owner[i], r = limbs[i];
      seg[((size_t)w * mh::SPLIT_MAX_SEG + S.n_seg[w]) * 2] = r, seg[((size_t)w * mh::SPLIT_MAX_SEG + S.n_seg[w]) * 2 + 1] = r + cnt[r];
      S.n_seg[w]++;
      if (MI(r, mh::MI_PARENT) >= 0)
         xslot[r] = slots, slots += 27;
   }
   for (int e = 0; e < n; e++)
      if (trunk[e])
         trunk_list.push_back(e);
   // adapted records: (body, field, value) triples applied on top of the model's records
   std::vector<int> nflags(n), nva(n, -1), nia(n, -1);
   for (int e = 0; e < n; e++)
      nflags[e] = MI(e, mh::MI_FLAGS);
   for (int e = 0; e < n; e++)
   {
      if (xslot[e] >= 0)
         nflags[e] &= ~mh::MF_PARENT_ADJ; // a limb root: its parent's state comes from the workspace, its contribution goes to the exchange record
      if (!trunk[e])
         continue;
      bool limb_child = false, nonadj_trunk_child = false;
      int first_acc = -1;
      for (int c : ch[e])
      {
         if (!trunk[c])
            limb_child = true;
         else if (c != e + 1)
            nonadj_trunk_child = true, first_acc = std::max(first_acc, c);
      }
      nflags[e] &= ~(mh::MF_HAS_ACC | mh::MF_STORE_VA);
      if (nonadj_trunk_child)
         nflags[e] |= mh::MF_HAS_ACC;
      if (limb_child || nonadj_trunk_child)
      {
         nflags[e] |= mh::MF_STORE_VA;
         if (!(MI(e, mh::MI_FLAGS) & mh::MF_STORE_VA))
            nva[e] = slots, slots += 12; // the model's records hold no slots for it
      }
      if (nonadj_trunk_child && !(MI(e, mh::MI_FLAGS) & mh::MF_HAS_ACC))
         nia[e] = slots, slots += 40;
      for (int c : ch[e])
         if (trunk[c] && c != e + 1) // first contributor of the trunk-only fold: the highest index
            nflags[c] = (nflags[c] & ~mh::MF_ACC_FIRST) | (c == first_acc ? mh::MF_ACC_FIRST : 0);
   }
   S.patches.clear();
   auto patch = [&](int e, int field, int value) { S.patches.push_back(e), S.patches.push_back(field), S.patches.push_back(value); };
   std::vector<int> xl_ofs(trunk_list.size() + 1, 0), xl;
   for (int e = 0; e < n; e++)
   {
      patch(e, mh::MI_HAND, xslot[e]);
      patch(e, mh::MI_FLAGS, nflags[e]);
      if (nva[e] >= 0)
         patch(e, mh::MI_SLOT_VA, nva[e]);
      if (nia[e] >= 0)
         patch(e, mh::MI_SLOT_IA, nia[e]);
   }
   for (size_t k = 0; k < trunk_list.size(); k++)
   {
      for (size_t i = 0; i < limbs.size(); i++)
         if (MI(limbs[i], mh::MI_PARENT) == trunk_list[k])
            xl.push_back(xslot[limbs[i]]);
      xl_ofs[k + 1] = (int)xl.size();
   }
   if (xl.empty())
      xl.push_back(0);
   if (trunk_list.empty())
      trunk_list.push_back(0);
   S.n_trunk = best_ntc, S.n_limbs = (int)limbs.size(), S.slots = slots, S.est = (S.est + 5) / 10, S.total = (sz_total + 5) / 10;
   S.trunk_list = trunk_list, S.seg = seg, S.xl_ofs = xl_ofs, S.xl = xl;
   S.usable = true;
   return S;
}
// Record set k of a usable split ([0] fp32, [1] fp64, [2] no LDS share): the adapted body records -- the model's with the (body, field,
// value) patches of the plan applied, then every workspace slot number turned into a slot CODE (home bit) for the precision's LDS share
// -- and the exchange slots coded the same way.  Slots below lds_slots live in LDS (the slot codes of the records say so).
struct SplitRecords
{
   int lds_slots = 0;
   std::vector<int> meta, xl;
};
SplitRecords split_rt_records(const SplitPlan &S, const std::vector<int> &model_meta, int n, int k)
{
   static const int slot_fields[] = {mh::MI_SLOT_JP, mh::MI_SLOT_F, mh::MI_SLOT_VA, mh::MI_SLOT_C, mh::MI_SLOT_IA, mh::MI_SLOT_LK, mh::MI_HAND};
   SplitRecords R;
   const long elem = k == 0 ? 4 : 8;
   const long cap = 160 * 1024 / (64 * elem);
   R.lds_slots = k == 2 ? 0 : (int)(S.slots <= cap ? S.slots : cap - mh::SPLIT_LDS_MARGIN); // everything, or a share with room for a group
   std::vector<int> meta = model_meta;
   for (size_t i = 0; i + 2 < S.patches.size(); i += 3)
      meta[(size_t)S.patches[i] * mh::MI_STRIDE + S.patches[i + 1]] = S.patches[i + 2];
   auto code = [&](int slot) { return slot >= 0 && slot < R.lds_slots ? (slot | mh::DFS_LDS) : slot; };
   for (int e = 0; e < n; e++)
      for (int f : slot_fields)
         meta[(size_t)e * mh::MI_STRIDE + f] = code(meta[(size_t)e * mh::MI_STRIDE + f]);
   std::vector<int> xl = S.xl;
   for (int &x : xl)
      x = code(x);
   R.meta = std::move(meta), R.xl = std::move(xl);
   return R;
}
// Workgroups of a run-time tree-split launch: single calls put `wgs` on every CU at most; the pair call (split_rt_shape with pair) one per
// algorithm and group of 64 configurations, taken while they fit the CUs.  Each has a workspace block of its own.
int split_rt_grid(int cu_count, int64_t B, int wgs) { return (int)std::max<long>(1, std::min<long>(groups_of(B), (long)cu_count * wgs)); }
size_t split_rt_ws_bytes(int slots, long grid, size_t elem) { return (size_t)slots * (size_t)grid * 64 * elem; }
// The shape of such a launch: record set, kernel build (0: every slot in LDS, 1: none, 2: a share), dynamic LDS bytes, grid.
// slots, lds_slots: SplitPlan::slots and SplitRecords::lds_slots of the three record sets; elem: sizeof(T)
struct SplitShape
{
   int k, mode, grid;
   size_t lds;
};
SplitShape split_rt_shape(int slots, const int lds_slots[3], int cu_count, size_t elem, Algo algo, int64_t B, bool pair)
{
   SplitShape s{};
   const long groups = groups_of(B);
   // workgroups per CU: the fp64 ABA holds ~300 registers (one wave per SIMD), the others fit two workgroups (measured on the humanoid at
   // B = 32768, two groups per CU: RNEA 47 us with two resident workgroups against 66 looping one; round 2, DESIGN_HISTORY.md)
   const int grid = pair ? (int)(2 * groups) : split_rt_grid(cu_count, B, (algo == ALGO_ABA && elem == 8) ? 1 : 2);
   // Which record set: everything in LDS when the block fits (no branches); else a share in LDS once the blocks of the workgroups of an
   // XCD outgrow its L2 (measured on the fp64 humanoid: 44 us all-global vs 47 with a share at B = 4096, 71 vs 50 at 8192); else all global.
   // The pair call keys on its groups: it then takes the record set (hence the kernel instantiation) of the single calls of its batch, and
   // the two agree bit for bit with it (its grid never exceeds the CUs).
   const long key = pair ? groups : grid;
   int k = elem == 4 ? 0 : 1;
   if (lds_slots[k] < slots && (size_t)slots * 64 * elem * ((size_t)key / 8 + 1) <= (size_t)3 << 20)
      k = 2;
   if (grid > cu_count && (size_t)std::min(slots, lds_slots[k] + mh::SPLIT_LDS_MARGIN) * 64 * elem > 80 * 1024)
      k = 2; // two workgroups per CU: an LDS share above half the CU's would serialise them
   s.k = k, s.grid = grid;
   s.mode = lds_slots[k] >= slots ? 0 : (lds_slots[k] == 0 ? 1 : 2);
   s.lds = s.mode == 1 ? 0 : (size_t)std::min(slots, lds_slots[k] + mh::SPLIT_LDS_MARGIN) * 64 * elem;
   return s;
}

// ---- frictional contact solve (mh_contact_kernels.h): where the sweeps read S.  The lower block triangle of S is 9 K (K + 1) / 2 entries
// per lane; a wave (one workgroup) keeps it in LDS while that fits the 160 KB of a CU -- 46 KB at K = 4 in fp64, 83 KB at K = 8 in fp32;
// 166 KB at K = 8 in fp64 do not -- and otherwise streams it from W in the SoA scratch.  force: -1 = choose, 0 = stream, 1 = resident
// where it fits (tests and measurements: both forms give the same bits).  The grid: the waves of the batch, capped at what is resident per
// CU -- the kernel's registers allow two waves per SIMD, the LDS copy floor(160 KB / bytes) workgroups.
struct ContactPlan
{
   bool resident;
   long lds;
   int per_cu, grid, kmax;
};
ContactPlan contact_plan(int K, size_t elem, int force, int cu_count, int64_t B)
{
   ContactPlan p{};
   const long bytes = 9L * K * (K + 1) / 2 * 64 * (long)elem;
   p.resident = force != 0 && bytes <= 160 * 1024;
   p.lds = p.resident ? bytes : 0;
   p.per_cu = p.resident ? (int)std::max<long>(1, std::min<long>(kWavesPerCu, 160 * 1024 / bytes)) : kWavesPerCu;
   p.grid = (int)std::max<long>(1, std::min<long>(groups_of(B), (long)cu_count * p.per_cu));
   p.kmax = K <= 4 ? 4 : 8; // the kernel build: contacts the unrolled loops cover
   return p;
}

// ---- joint-limit solve (mh_limit_kernels.h): a wave (one workgroup) keeps t, c and rho of its L rows in LDS, 3 L entries per lane, and
// the lower triangle of the listed block of H^-1, L (L + 1) / 2 entries per lane, behind them while both fit the 160 KB of a CU -- up to
// L = 22 in fp64 (163 328 bytes; L = 23 takes 176 640), up to L = 32 in fp32 -- and otherwise streams the triangle from the columns in
// the SoA scratch.  force: -1 = choose, 0 = stream, 1 = resident where it fits (tests and measurements: both forms give the same bits).
// The grid: the waves of the batch, capped at the workgroups whose LDS a CU holds, eight at most.
struct LimitPlan
{
   bool resident;
   long lds;
   int per_cu, grid;
};
LimitPlan limit_plan(int L, size_t elem, int force, int cu_count, int64_t B)
{
   LimitPlan p{};
   const long state = 3L * L * 64 * (long)elem, full = state + (long)L * (L + 1) / 2 * 64 * (long)elem;
   p.resident = force != 0 && full <= 160 * 1024;
   p.lds = p.resident ? full : state;
   p.per_cu = (int)std::max<long>(1, std::min<long>(kWavesPerCu, 160 * 1024 / p.lds));
   p.grid = (int)std::max<long>(1, std::min<long>(groups_of(B), (long)cu_count * p.per_cu));
   return p;
}

// ---- the constrained and the contact dynamics (mh_constraint_kernels.h, mh_contact_kernels.h), rooted and _between_ forms alike: the
// frames their inverse apparent inertia W is taken at, and where the launches of one call keep their scratch
constexpr double kIdentityPose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}; // R row-major, then p
double rotation_error(const double *X)
{
   const double det = X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6]) + X[2] * (X[3] * X[7] - X[4] * X[6]);
   double worst = std::fabs(det - 1.0);
   for (int r = 0; r < 3; r++)
      for (int s = 0; s < 3; s++)
      {
         double g = 0.0;
         for (int t = 0; t < 3; t++)
            g += X[3 * t + r] * X[3 * t + s];
         worst = std::max(worst, std::fabs(g - (r == s ? 1.0 : 0.0)));
      }
   return worst; // (NaN where an entry is)
}
// The frame of a target in the canonical after-joint frame of its body: (body-fixed -> canonical) o (target frame -> body-fixed), where
// X (NULL: the identity) is the caller's pose of the target frame in the body-fixed frame of engine body e; e = -1 is the root body,
// whose body-fixed frame is the root frame itself.  Refused, as target k of `call` (NULL: none named), where the 3 x 3 part of X is no rotation (NaN too).
template <typename T>
mh_status target_frame(const ModelTables *m, int e, const double *X, T pose[12], const char *call, int k)
{
   static_assert(mh::MC_PF == mh::MC_RF + 9, "the body-fixed frame's rotation and translation are one pose of 12 numbers");
   if (!X)
      X = kIdentityPose;
   const double off = rotation_error(X);
   if (!(off <= 1.0e-9))
      return call ? fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d: the 3 x 3 part of its pose is not a rotation (off by %.3g > 1e-9)", call, k, off)
                  : fail(MH_ERR_INVALID_ARGUMENT, "target %d: the 3 x 3 part of its pose is not a rotation (off by %.3g > 1e-9)", k, off);
   const double *c = e < 0 ? kIdentityPose : &m->consts[(size_t)e * mh::MC_STRIDE + mh::MC_RF];
   for (int r = 0; r < 3; r++)
   {
      double p = c[9 + r];
      for (int t = 0; t < 3; t++)
         p += c[3 * r + t] * X[9 + t];
      pose[9 + r] = (T)p;
      for (int s = 0; s < 3; s++)
      {
         double v = 0.0;
         for (int t = 0; t < 3; t++)
            v += c[3 * r + t] * X[3 * t + s];
         pose[3 * r + s] = (T)v;
      }
   }
   return MH_OK;
}
// The frames of one call (FrameList F{K, K}): K targets, each held against a base; W's: the targets, then the body-fixed frame of every non-root base
static_assert(MH_MAX_CONSTRAINT_TARGETS == MH_MAX_CONTACT_TARGETS && 2 * MH_MAX_CONSTRAINT_TARGETS <= MH_MAX_APPARENT_TARGETS, "one list serves both");
struct FrameList
{
   static constexpr int N = MH_MAX_CONSTRAINT_TARGETS, M = MH_MAX_APPARENT_TARGETS;
   int K, n_app;                                   // targets; frames of W
   int tgt[N], ext[N], base[N], bext[N], bslot[N]; // per target, as ConRelArgs and ContactRelArgs hold them (mh_constraint_kernels.h),
   double pose[N][12];                             // and its pose as the caller gave it
   int32_t app_joints[M];                          // per frame of W: its joint in the caller's order,
   double app_canon[M][12];                        // and its pose in the canonical frame of its body (target_frame)
};
// Target k < K of the list, by its joint and its base's in the caller's order; its pose from `poses` ([K][12], NULL: identities), which the
// caller checks after its own checks of the target (target_frame of pose[k] into app_canon[k]).  contact: the noun of the own-body refusal.
mh_status frame_target(const ModelTables &m, FrameList &F, int k, int joint, int base_joint, const double *poses, const char *call, bool contact)
{
   if (joint < 0 || joint >= m.n)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d names joint %d (the model has %d joints; the root body is no target)", call, k, joint, m.n);
   if (base_joint < -1 || base_joint >= m.n)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: base %d names joint %d (the model has %d joints; -1 is the root body)", call, k, base_joint, m.n);
   if (base_joint == joint)
      return contact ? fail(MH_ERR_INVALID_ARGUMENT, "%s: contact %d is between a body and itself (joint %d): the Jacobian is zero", call, k, joint)
                     : fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d is held against its own body (joint %d): the Jacobian is zero", call, k, joint);
   F.tgt[k] = m.engine_of[joint], F.ext[k] = F.app_joints[k] = joint;
   F.base[k] = base_joint < 0 ? -1 : m.engine_of[base_joint], F.bext[k] = base_joint, F.bslot[k] = -1;
   std::copy_n(poses ? poses + 12 * k : kIdentityPose, 12, F.pose[k]);
   return MH_OK;
}
// Closes a list whose K targets are resolved: one more frame of W per non-root base
void frame_list_close(const ModelTables &m, FrameList &F)
{
   for (int k = 0; k < F.K; k++)
      if (F.base[k] >= 0)
      {
         assert(F.n_app < MH_MAX_APPARENT_TARGETS); // K targets and at most one base each: n_app <= 2 K <= MH_MAX_APPARENT_TARGETS
         F.app_joints[F.bslot[k] = F.n_app++] = F.bext[k];
         target_frame<double>(&m, F.base[k], nullptr, F.app_canon[F.bslot[k]], nullptr, k);
      }
}
// The scratch of one call (mh_model::con), blocks of [entries][B]: offsets and total per configuration, in elements, with the totals of
// include/mecano_hip.h.  zpose and twist exist only with a base that is not the root (n_app > K), twist only where the call wants it.
struct ConScratch
{
   size_t W, rhs, body, wrench, zeros, zpose, twist, total;
};
ConScratch con_scratch(int n_joints, int nv, int K, int n_app, bool wants_twists)
{
   const size_t n6 = 6 * (size_t)n_joints, rel = n_app > K;
   const size_t rhs = 36 * (size_t)n_app * n_app, body = rhs + 6 * (size_t)K, zeros = body + 2 * n6, zpose = zeros + (size_t)nv, twist = zpose + rel * 12 * (size_t)K;
   return {0, rhs, body, body + n6, zeros, zpose, twist, twist + (rel && wants_twists ? n6 : 0)};
}
} // namespace
