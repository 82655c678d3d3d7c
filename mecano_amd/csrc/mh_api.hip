// mh_api.hip -- host side of the C-ABI declared in include/mecano_hip.h.
//
// Model build (once per MultiBodySystemReadOnly): validation, parents-first ordering, canonical joint frames,
// workspace slot assignment (all host arithmetic: mh_model_tables.h), upload.  Compute calls: argument checks, workspace, kernel launch on the caller's
// stream.  No CPU implementation of the algorithms exists in this library: without a HIP device the compute
// entry points return MH_ERR_NO_DEVICE.
#include "../../include/mecano_hip.h"
#include "mh_dfs_kernels.h"
#include "mh_split_kernels.h"
#include "mh_gravity_kernels.h"
#include "mh_response_kernels.h"
#include "mh_minv_kernels.h"
#include "mh_kinematics_kernels.h"
#include "mh_kinematics_vjp_kernels.h"
#include "mh_rnea_deriv_kernels.h"
#include "mh_params_kernels.h"
#include "mh_params_vjp_kernels.h"
#include "mh_params_state_vjp_kernels.h"
#include "mh_step_kernels.h"
#include "mh_constraint_kernels.h"
#include "mh_contact_kernels.h"
#include "mh_limit_kernels.h"
#include "mh_model_tables.h"
#include "mh_launch_plans.h"

#include <dlfcn.h>
#include <spawn.h>
#include <sys/wait.h>
#include <unistd.h>
#include <cerrno>
extern char **environ;
#include <unistd.h>

#include <algorithm>
#include <functional>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

namespace
{
#define HIP_TRY(expr)                                                                                      \
   do                                                                                                      \
   {                                                                                                       \
      hipError_t e_ = (expr);                                                                              \
      if (e_ != hipSuccess)                                                                                \
         return fail(e_ == hipErrorOutOfMemory ? MH_ERR_OUT_OF_MEMORY : MH_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
   } while (0)

// NaN tests on raw 64-bit words that never pass through a `double` value: this translation unit is built with -ffinite-math-only, under
// which x != x folds to false AND double parameters carry nofpclass(nan), so that even a bit test on a double argument may be folded away
inline bool nan_word(unsigned long long u) { return (u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && (u & 0x000fffffffffffffull) != 0; }
inline bool nonfinite_word(unsigned long long u) { return (u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull; }
inline bool nonfinite_bits(const double &x)
{
   unsigned long long u;
   std::memcpy(&u, (const void *)&x, sizeof u);
   asm volatile("" : "+r"(u));
   return nonfinite_word(u);
}
inline bool nan_bits(const double &x)
{
   unsigned long long u;
   std::memcpy(&u, (const void *)&x, sizeof u);
   asm volatile("" : "+r"(u)); // the optimiser must not trace the word back to a floating-point value
   return nan_word(u);
}
// ---- build provenance (mecano_amd/build.py computes the same numbers): FNV-1a 64 over, per file, name 0 contents 0, then the
//      code-generation flags.  The library carries the hash of its own sources (MH_BUILD_HASH) and the hash it expects of a code
//      object's sources (MH_SPEC_SOURCES_HASH); a code object carries the latter and is refused when it differs (try_load_spec).
#define MH_STR2_(...) #__VA_ARGS__
#define MH_STR_(...) MH_STR2_(__VA_ARGS__)
#ifndef MH_BUILD_HASH
#define MH_BUILD_HASH unhashed
#endif
#ifndef MH_SPEC_SOURCES_HASH
#define MH_SPEC_SOURCES_HASH unhashed
#endif
__attribute__((used)) const char kBuildId[] = "MH_BUILD_ID=" MH_STR_(MH_BUILD_HASH) ";spec=" MH_STR_(MH_SPEC_SOURCES_HASH) ";";
const char *const kSpecHashFiles[] = {"mh_spec.hip", "mh_spec_kernels.h", "mh_zv_kernels.h", "mh_kernels.h", "mh_device.h"};
const char kSpecCodegenFlags[] = "--offload-arch=gfx950 -O3 -std=c++17 -fno-signed-zeros -ffinite-math-only -fno-slp-vectorize -mllvm -disable-machine-licm";
uint64_t fnv1a(uint64_t h, const void *data, size_t n)
{
   const unsigned char *p = (const unsigned char *)data;
   for (size_t k = 0; k < n; k++)
      h = (h ^ p[k]) * 0x100000001b3ull;
   return h;
}
bool hash_spec_sources(const std::string &csrc_dir, char out[18])
{
   uint64_t h = 0xcbf29ce484222325ull;
   for (const char *name : kSpecHashFiles)
   {
      FILE *f = fopen((csrc_dir + "/" + name).c_str(), "rb");
      if (!f)
         return false;
      h = fnv1a(h, name, strlen(name) + 1);
      char buf[1 << 16];
      size_t got;
      while ((got = fread(buf, 1, sizeof buf, f)) > 0)
         h = fnv1a(h, buf, got);
      fclose(f);
      h = fnv1a(h, "", 1);
   }
   h = fnv1a(h, kSpecCodegenFlags, sizeof kSpecCodegenFlags - 1);
   snprintf(out, 18, "h%016llx", (unsigned long long)h);
   return true;
}

struct Workspace
{
   void *ptr = nullptr;
   size_t bytes = 0;
};
// A member of mh_model that a compute call may be WRITING while another thread copies the model into a new context
// (mh_context_create): the copy never reads it -- it starts empty, which is what a context wants anyway.
template <class T>
struct FreshOnCopy : T
{
   FreshOnCopy() = default;
   FreshOnCopy(const FreshOnCopy &) : T() {}
   FreshOnCopy &operator=(const FreshOnCopy &) { return *this; }
   FreshOnCopy &operator=(const T &v)
   {
      T::operator=(v);
      return *this;
   }
};
std::mutex g_error_words_mutex;
std::vector<int *> g_error_words; // every live model's / context's mapped error word (mh_stream_synchronize has no handle to ask)

// Everything compute calls write: owned by a model (its default context) and by every context (mh_context_create).  Declared, defaulted
// and released HERE only: a member added to this struct is a context's own without another line anywhere.
struct ContextState
{
   Workspace ws;
   // mh_rnea_aba_f64 without a fused kernel, small batches: the two launches run side by side, the ABA on this stream with its own workspace
   Workspace ws_pair;
   hipStream_t pair_stream = nullptr;
   hipEvent_t pair_fork = nullptr, pair_join = nullptr;
   // staging buffers of the *_host entry points
   Workspace stage;
   // pipelined host path: copy-in / compute / copy-out streams and per-slot events of a ring of three device chunk slots
   hipStream_t hs_in = nullptr, hs_run = nullptr, hs_out = nullptr;
   hipEvent_t ev_in[3] = {}, ev_run[3] = {}, ev_out[3] = {};
   // AoS -> SoA scratch copies of the state matrices for the run-time-topology kernels (big batches of wide matrices); tr_pair: the
   // copies of the forward dynamics call that runs beside the inverse dynamics call on pair_stream (they would share addresses otherwise)
   Workspace tr, tr_pair;
   // scratch of the composite entry points: efforts of the Newton-Euler sweep behind mh_aba_joint_wrenches_f64, pair lists of
   // mh_relative_acceleration_f64
   Workspace aux, pairs;
   FreshOnCopy<std::vector<int>> pairs_host;
   // mh_rnea_derivatives_* / mh_aba_derivatives_*: scratch of the forward form (Hinv and qdd the caller did not ask for)
   Workspace deriv;
   // mh_aba_vjp_* / mh_aba_parameters_vjp_* / mh_aba_parameters_state_vjp_*: qdd and H^-1 w the caller did not ask for, B nv entries each
   Workspace vjp;
   // mh_aba_integrate_derivatives_*: d qdd / d q and d qdd / d qd of the call (Hinv and qdd go to `deriv`)
   Workspace step;
   // mh_body_poses_* / mh_geometric_jacobian_*: the SoA form of AoS outputs, which a transposition then brings to the caller's rows
   // (mh_body_poses_vjp_* / mh_jacobian_transpose_*: the SoA form of their AoS cotangents too)
   Workspace kin;
   // mh_aba_constrained_* / mh_constraint_impulse_* / mh_contact_impulse_* and their _between_ forms: the blocks of con_scratch
   // (mh_launch_plans.h)
   Workspace con;
   // bias-split forward dynamics (mh_zv_kernels.h): tau - h(q, qd) rows, one flag per 64 configurations (a launch stores its epoch there),
   // an error word in mapped host memory that a timed-out wait sets (read at the next call of the model)
   Workspace zv_tau, zv_flags;
   Workspace zv_cols;     // two-stage hand-off with self-signalling limb columns (identity index maps): [groups][nv][64], holds the sentinel
                          // between launches (mh_zv_kernels.h: ZV_SENTINEL) -- written by nothing but those launches
   Workspace zvb_cs;      // two-launch forward dynamics: (cos, sin) of the revolute joints, [2 n_rev][B rounded up to 64]
   int zv_epoch = 0;
   int *zv_error_host = nullptr, *zv_error_dev = nullptr;
   FreshOnCopy<std::map<const void *, size_t>> lds_attr; // dynamic-LDS limit already raised per kernel (the model lives on one device, one host thread at a time)
};
void free_scratch(ContextState &c)
{
   for (Workspace *w : {&c.ws, &c.ws_pair, &c.stage, &c.tr, &c.tr_pair, &c.aux, &c.pairs, &c.deriv, &c.vjp, &c.step, &c.kin, &c.con, &c.zv_tau, &c.zv_flags, &c.zv_cols, &c.zvb_cs})
      (void)hipFree(w->ptr);
   if (c.zv_error_host)
   {
      {
         std::lock_guard<std::mutex> lock(g_error_words_mutex);
         g_error_words.erase(std::remove(g_error_words.begin(), g_error_words.end(), c.zv_error_host), g_error_words.end());
      }
      (void)hipHostFree(c.zv_error_host);
   }
   if (c.pair_stream)
   {
      (void)hipStreamDestroy(c.pair_stream);
      (void)hipEventDestroy(c.pair_fork);
      (void)hipEventDestroy(c.pair_join);
   }
   for (hipEvent_t e : {c.ev_in[0], c.ev_in[1], c.ev_in[2], c.ev_run[0], c.ev_run[1], c.ev_run[2], c.ev_out[0], c.ev_out[1], c.ev_out[2]})
      if (e)
         (void)hipEventDestroy(e);
   for (hipStream_t s : {c.hs_in, c.hs_run, c.hs_out})
      if (s)
         (void)hipStreamDestroy(s);
}

// The device copies of a model's tables: one member here and one row in device_rows() -- upload (mh_model_create) and release
// (release_model) walk that list.  A context shares its model's (mh_context_create).
struct DeviceTables
{
   int *d_meta = nullptr, *d_dof = nullptr, *d_cfg = nullptr, *d_prog = nullptr, *d_prog_seq = nullptr;
   double *d_consts64 = nullptr;
   float *d_consts32 = nullptr;
   double *d_sub_mass64 = nullptr;
   float *d_sub_mass32 = nullptr;
   int *d_grav_zero_ofs = nullptr, *d_grav_zero_cols = nullptr;
   int *d_resp_info = nullptr;
   int *d_minv_owner = nullptr;
   int *d_deriv_slot = nullptr;
   int *d_vjp_slot = nullptr;
   int *d_jvp_slot = nullptr;
};

// The switches of the environment (struct Switches: mh_launch_plans.h, whose planners read some of them).
// Every switch keeps its default where its variable is unset.  mh_model_create calls this AFTER it has put the device's CU count and the
// bushiness heuristic into cu_count and dfs_aba64: MH_FAKE_CU_COUNT and MH_DFS_ABA64 override those.
void read_switches(Switches &s)
{
   auto set = [](const char *e, auto &member, auto parse) {
      if (e)
         member = parse(e);
   };
   auto number = [](const char *e) { return atoi(e); };
   auto boolean = [](const char *e) { return atoi(e) != 0; };
   auto at_least_0 = [](const char *e) { return std::max(0, atoi(e)); };
   set(getenv("MH_DISABLE_SPEC"), s.use_spec, [](const char *e) { return atoi(e) ? 0 : 1; });
   set(getenv("MH_SPEC_SPLIT"), s.use_split, number);
   set(getenv("MH_ZV"), s.use_zv, number);
   set(getenv("MH_ZV_SAME_L2"), s.zv_same_l2, boolean);
   set(getenv("MH_ZV_WAIT_MS"), s.zv_wait_ticks, [](const char *e) { return (unsigned)std::max<long long>(1, std::min<long long>(40000, atoll(e))) * 100000u; });
   set(getenv("MH_ZVB"), s.use_zvb, number);
   set(getenv("MH_ZVF"), s.use_zvf, number);
   set(getenv("MH_ZVF_PAIR"), s.use_zvf_pair, number);
   set(getenv("MH_RNEA_AHEAD"), s.use_rnea_ahead, number);
   set(getenv("MH_ZV_STEP"), s.use_zv_step, boolean);
   set(getenv("MH_ZVB_WHICH"), s.zvb_which, [](const char *e) { return std::max(1, std::min(3, atoi(e))); });
   set(getenv("MH_SPEC_IO"), s.force_io, number);
   set(getenv("MH_FAKE_CU_COUNT"), s.cu_count, [](const char *e) { return std::max(1, atoi(e)); });
   set(getenv("MH_GENERIC_TRANSPOSE"), s.use_transpose, boolean);
   set(getenv("MH_SPEC_ST"), s.force_st, number);
   set(getenv("MH_DFS"), s.use_dfs, boolean);
   set(getenv("MH_DFS_PAIR"), s.use_dfs_pair, boolean);
   set(getenv("MH_DFS_ABA64"), s.dfs_aba64, boolean);
   set(getenv("MH_DFS_BUDGET"), s.dfs_budget, at_least_0);
   set(getenv("MH_DFS_PLACE"), s.dfs_place, number);
   set(getenv("MH_DFS_GREEDY"), s.dfs_place_greedy, boolean);
   set(getenv("MH_HOST_CHUNK"), s.host_chunk, at_least_0);
   set(getenv("MH_SPLIT_RT"), s.use_split_rt, number);
}
} // namespace

// entry points of a topology-specialised code object (mh_spec.hip), resolved with dlsym
struct SpecLib
{
   void *handle = nullptr;
   int (*launch)(int algo, int flags, const void *args, int grid, void *stream) = nullptr;
   long (*lds_bytes)(int algo, int flags, int nq, int nv) = nullptr;
   int (*aba_slots)(void) = nullptr;
   int (*supports)(int algo, int flags) = nullptr;
   int (*launch_fused)(int flags, const void *args, int waves, void *stream) = nullptr;
   long (*fused_lds_bytes)(int nq, int nv) = nullptr;
   int (*launch_crba)(int flags, const void *args, int grid, void *stream) = nullptr;
   int (*crba_packed)(int flags) = nullptr;
   int (*split_usable)(void) = nullptr;
   long (*split_lds_bytes)(int algo, int flags, int nq, int nv) = nullptr;
   int (*launch_split)(int algo, int flags, const void *args, int groups, void *stream) = nullptr;
   int (*crba_split_usable)(void) = nullptr;
   int (*launch_crba_split)(const void *args, int groups, int lanes_per_group, void *stream) = nullptr;
   int (*launch_rnea_crba)(const void *args, int rnea_groups, int crba_groups, int lanes_per_group, void *stream) = nullptr;
   long (*rnea_crba_lds_bytes)(int lanes_per_group, int nq, int nv) = nullptr;
   int (*launch_coriolis)(int flags, const void *args, int grid, void *stream) = nullptr;
   int (*launch_centroidal)(int flags, const void *args, int grid, void *stream) = nullptr;
   int (*launch_coriolis_parts)(int flags, const void *args, int grid, int parts, void *stream) = nullptr;
   int (*launch_centroidal_parts)(int flags, const void *args, int grid, int parts, void *stream) = nullptr;
   unsigned long long (*abi)(void) = nullptr;
   const char *(*sources_hash)(void) = nullptr;
   // bias-split forward dynamics (mh_zv_kernels.h)
   int (*zv_usable)(void) = nullptr;
   long (*zv_lds_bytes)(int nq, int nv) = nullptr;
   int (*launch_zv)(int flags, const void *args, void *taup, int *sync_flags, int *error, int epoch, int jobs, int same_l2, unsigned wait_ticks, void *stream) = nullptr;
   int (*zv_self_signal)(void) = nullptr; // 1: identity-map launches expect taup to hold the sentinel wherever no column has been published
   // forward dynamics of device-filling batches as two launches (mh_zv_kernels.h, spec_zvb_*)
   int (*zvb_usable)(void) = nullptr;
   int (*zvb_cs_rows)(void) = nullptr;
   long (*zvb_lds_bytes)(int which, int nq, int nv) = nullptr;
   int (*launch_zvb)(int flags, const void *args, void *taup, void *cs, long cs_stride, int groups, int which, void *stream) = nullptr;
   // ... as one launch, both jobs fused in a workgroup (spec_zvf_kernel)
   int (*zvf_usable)(void) = nullptr;
   int (*zvf_pair_usable)(void) = nullptr; // 1: launch_zvf serves the pair call too (args->in3b = qdd, args->outb = tau)
   int (*launch_zvf)(int flags, const void *args, int groups, void *stream) = nullptr;
   int (*launch_rnea_ahead)(int flags, const void *args, int groups, void *stream) = nullptr;
};
enum : int
{
   SPEC_IO_LDS = 1,
   SPEC_IDENT = 2,
   SPEC_ST_LDS = 4,
   SPEC_BODIES = 16,
   SPEC_OCC3 = 32
};

// A model is four things, each stated once: what mh_model_create compiles from the description (ModelTables, mh_model_tables.h), its copies
// on the device, the switches of the environment, and what compute calls write.  Declared here: lifecycle, code object and launch plans.
struct mh_model : ModelTables, DeviceTables, Switches, ContextState
{
   int device = 0;
   // mh_context_create: a context is a copy of the model's host-side description that SHARES its device records (parent owns them) and
   // owns everything compute calls write -- a ContextState of its own
   mh_model *parent = nullptr;
   int n_contexts = 0; // live contexts of this model (guarded by g_context_mutex)
   bool destroy_pending = false; // mh_model_destroy was called while contexts were alive: the last mh_context_destroy releases the model
   int n_locked = 0;        // joints in MH_ACCELERATION_SOURCE mode (mh_model_set_joint_source_modes)
   // mh_rnea_vjp_* / mh_aba_vjp_*: first workspace slot of every body in that kernel's own plan (vjp_slot_plan, mh_launch_plans.h)
   std::vector<int> vjp_slot;
   int vjp_slots = 0;
   // mh_rnea_jvp_* / mh_aba_jvp_*: the same for the tangent sweep (jvp_slot_plan)
   std::vector<int> jvp_slot;
   int jvp_slots = 0;
   SpecLib spec;
   bool spec_minimal = false; // the loaded code object is a minimal (fast) build
   std::string variant = "generic";
   // depth-first kernels: frame homes for a given LDS budget (slots per wave), one copy of the body records per (algorithm, budget) on
   // the device; built on first use (dfs_plan), dropped when the records change (joint source modes)
   struct DfsPlan
   {
      int algo, budget, lds_slots, glb_slots, glb_frames;
      int *d_meta;
   };
   FreshOnCopy<std::deque<DfsPlan>> dfs_plans; // references stay valid across push_back; kept by the model itself (a context uses its model's: dfs_plan)
   struct PlainMutex : std::mutex
   { // a context starts as a copy of its model (context_clone): the copy gets a mutex of its own
      PlainMutex() = default;
      PlainMutex(const PlainMutex &) : std::mutex() {}
      PlainMutex &operator=(const PlainMutex &) { return *this; }
   } dfs_mutex;
   // run-time tree split (mh_split_kernels.h): plan made at creation (mh_launch_plans.h), device copies (split_rt_rows)
   struct SplitRt : SplitPlan
   {
      int *d_meta[3] = {nullptr, nullptr, nullptr}, *d_trunk = nullptr, *d_seg = nullptr, *d_xl_ofs = nullptr, *d_xl[3] = {nullptr, nullptr, nullptr}; // [0] fp32, [1] fp64, [2] no LDS share
      int lds_slots[3] = {0, 0, 0}; // slots below this number live in LDS (the slot codes of the records say so), per record set
   } split_rt;
};

struct mh_context
{
   mh_model *m; // the context's copy of the handle (parent = the model it was created from)
};
namespace
{
std::mutex g_context_mutex;
// The device tables of a model, in upload order: where the pointer lives and what it is a copy of.  consts and sub_mass go up twice, the
// fp32 copies made by the caller at upload (release_model reads the pointers only and passes none).
struct DeviceRow
{
   void **ptr;
   const void *host;
   size_t bytes;
};
template <class T>
DeviceRow device_row(T *&ptr, const std::vector<T> &host) { return DeviceRow{(void **)&ptr, host.data(), host.size() * sizeof(T)}; }
std::vector<DeviceRow> device_rows(mh_model *m, const std::vector<float> &consts32 = {}, const std::vector<float> &sub_mass32 = {})
{
   return {device_row(m->d_meta, m->meta), device_row(m->d_dof, m->dof_map), device_row(m->d_cfg, m->cfg_map), device_row(m->d_prog, m->prog),
           device_row(m->d_prog_seq, m->prog_seq), device_row(m->d_consts64, m->consts), device_row(m->d_consts32, consts32),
           device_row(m->d_sub_mass64, m->sub_mass), device_row(m->d_sub_mass32, sub_mass32), device_row(m->d_grav_zero_ofs, m->grav_zero_ofs),
           device_row(m->d_grav_zero_cols, m->grav_zero_cols), device_row(m->d_resp_info, m->resp_info),
           device_row(m->d_minv_owner, m->minv_owner), device_row(m->d_deriv_slot, m->deriv_slot), device_row(m->d_vjp_slot, m->vjp_slot),
           device_row(m->d_jvp_slot, m->jvp_slot)};
}
mh_status ensure_bytes(Workspace &w, size_t bytes)
{
   if (w.bytes >= bytes)
      return MH_OK;
   if (w.ptr)
      HIP_TRY(hipFree(w.ptr));
   w.ptr = nullptr, w.bytes = 0;
   HIP_TRY(hipMalloc(&w.ptr, bytes));
   w.bytes = bytes;
   return MH_OK;
}

// one launch for RNEA + ABA (and the tree-split RNEA / ABA of a code object) while 2 * ceil(B / 64) workgroups <= cu_count * kFusedFactor
constexpr int kFusedFactor = 4;
// whole-tree forward dynamics of a code object: hand-over in LDS while waves <= cu_count * kAbaLdsFactor
constexpr int kAbaLdsFactor = 1;

mh_status ensure_workspace(mh_model *m, int64_t B, size_t elem)
{
   Launch L = plan_launch(m->cu_count, B);
   return ensure_bytes(m->ws, (size_t)m->n_slots * (size_t)L.lanes * elem);
}

template <typename T>
mh::DevModel dev_model(const mh_model *m)
{
   mh::DevModel d;
   d.n = m->n, d.nq = m->nq, d.nv = m->nv, d.n_slots = m->n_slots;
   d.meta = m->d_meta, d.dof_map = m->d_dof, d.cfg_map = m->d_cfg;
   d.consts = sizeof(T) == 8 ? (const void *)m->d_consts64 : (const void *)m->d_consts32;
   d.prog = m->d_prog, d.n_events = (int)m->prog.size();
   d.rnea_stack = m->rnea_stack, d.aba_stack = m->aba_stack, d.aba_hand = m->aba_hand;
   return d;
}

// Root acceleration of a call: (0, -g) for the gravity vector, or opts->root_acceleration (angular, linear) when the caller set one
// (InverseDynamicsCalculator.java:343-348 / 413-427, ForwardDynamicsCalculator.java:259-264 / 330-343).  The kernels take minus the linear
// part in (gx, gy, gz) and the angular part in (rax, ray, raz).
template <class ARGS>
void set_root_acceleration(ARGS &A, const mh_options &o, const double *gravity)
{
   using T = decltype(A.gx);
   if (o.use_root_acceleration)
   {
      A.rax = (T)o.root_acceleration[0], A.ray = (T)o.root_acceleration[1], A.raz = (T)o.root_acceleration[2];
      A.gx = (T)-o.root_acceleration[3], A.gy = (T)-o.root_acceleration[4], A.gz = (T)-o.root_acceleration[5];
   }
   else
   {
      A.rax = T(0), A.ray = T(0), A.raz = T(0);
      A.gx = gravity ? (T)gravity[0] : T(0), A.gy = gravity ? (T)gravity[1] : T(0), A.gz = gravity ? (T)gravity[2] : T(0);
   }
}

// Also resolves opts->context: a compute call made with a context runs on the context's copy of the handle (its own workspace, scratch,
// streams, flags); `model` is switched to it here, before the entry point touches anything mutable.
mh_status check_common(mh_model_t &model, int64_t B, const mh_options *opts)
{
   if (!model)
      return fail(MH_ERR_INVALID_ARGUMENT, "model is NULL");
   if (opts && opts->context)
   {
      mh_model *c = ((mh_context *)opts->context)->m;
      if (c->parent != (model->parent ? model->parent : model))
         return fail(MH_ERR_INVALID_ARGUMENT, "opts->context belongs to another model");
      model = c;
   }
   if (B < 0)
      return fail(MH_ERR_BAD_DIMENSION, "negative batch size %lld", (long long)B);
   if (opts && opts->layout != MH_LAYOUT_AOS && opts->layout != MH_LAYOUT_SOA)
      return fail(MH_ERR_INVALID_ARGUMENT, "unknown layout %d", opts->layout);
   int cur = 0;
   if (hipGetDevice(&cur) != hipSuccess)
      return fail(MH_ERR_NO_DEVICE, "no usable HIP device");
   if (cur != model->device)
      return fail(MH_ERR_INVALID_ARGUMENT, "model lives on device %d but the calling thread's device is %d", model->device, cur);
   return MH_OK;
}
// The options of a compute call (the defaults where opts_in is NULL), checked by check_common -- which switches `model` to their context
mh_status begin_call(mh_model_t &model, int64_t B, const mh_options *opts_in, mh_options &opts)
{
   if (opts_in)
      opts = *opts_in;
   else
      mh_options_default(&opts);
   return check_common(model, B, &opts);
}


// ---- the aliasing contract of the compute calls (include/mecano_hip.h, "Aliasing").  Host-side pointer comparisons, made after the NULL
// checks and before anything is launched or allocated: a refused call leaves its outputs untouched.
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
   const char *a0 = (const char *)a, *b0 = (const char *)b;
   return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}
struct InRange
{
   const char *name;
   const void *p;
   size_t bytes;
};
struct OutRange
{
   const char *name;
   const void *p;
   size_t bytes;
   unsigned may_be; // bit i: the output may BE input i -- the same pointer and the same size
};
// An output may be at most one of the inputs its mask names; any other overlap with an input, and any overlap of two outputs, is refused.
// NULL pointers and empty ranges overlap nothing.
mh_status check_aliasing(const char *call, const InRange *ins, int n_ins, const OutRange *outs, int n_outs)
{
   for (int o = 0; o < n_outs; o++)
   {
      const char *is = nullptr;
      for (int i = 0; i < n_ins; i++)
      {
         if (!ranges_overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes))
            continue;
         const bool same = outs[o].p == ins[i].p && outs[o].bytes == ins[i].bytes;
         if (!same || !((outs[o].may_be >> i) & 1u))
            return fail(MH_ERR_INVALID_ARGUMENT, "%s: %s must not overlap %s%s", call, outs[o].name, ins[i].name,
                        same ? "" : ((outs[o].may_be >> i) & 1u) ? " (it may be that matrix itself, not a part of it)" : "");
         if (is)
            return fail(MH_ERR_INVALID_ARGUMENT, "%s: %s overlaps both %s and %s (it may be one input, not two)", call, outs[o].name, is, ins[i].name);
         is = ins[i].name;
      }
      for (int p = o + 1; p < n_outs; p++)
         if (ranges_overlap(outs[o].p, outs[o].bytes, outs[p].p, outs[p].bytes))
            return fail(MH_ERR_INVALID_ARGUMENT, "%s: the outputs %s and %s overlap", call, outs[o].name, outs[p].name);
   }
   return MH_OK;
}

// (batch stride, element stride) of a matrix with rows of n entries in the call's layout
void set_strides(long &bs, long &es, bool soa, int64_t B, long n) { bs = soa ? 1 : n, es = soa ? B : 1; }

// The kernel arguments every call fills alike: the model, the batch, the strides of state (q, v) and wrench-sized (f) rows.  With the
// gravity argument also the root acceleration and the Coriolis / acceleration switches.  The caller sets the pointers and any stride
// that differs.
template <typename T>
mh::Args<T> make_args(const mh_model *m, int64_t B, const mh_options &o)
{
   mh::Args<T> A{};
   A.m = dev_model<T>(m);
   A.B = B;
   const bool soa = o.layout == MH_LAYOUT_SOA;
   set_strides(A.q_bs, A.q_es, soa, B, m->nq);
   set_strides(A.v_bs, A.v_es, soa, B, m->nv);
   set_strides(A.f_bs, A.f_es, soa, B, (long)m->n * 6);
   return A;
}
template <typename T>
mh::Args<T> make_args(const mh_model *m, int64_t B, const mh_options &o, const double *gravity)
{
   mh::Args<T> A = make_args<T>(m, B, o);
   set_root_acceleration(A, o, gravity);
   A.coriolis = o.consider_coriolis, A.accel = o.consider_accelerations;
   return A;
}
// The set-up of a lane sweep whose bodies up to min(8, n) waves per group of configurations share: the launch shape, the workspace of
// `slots` entries per lane on every such wave, and the kernel's common arguments with the workspace in them.
template <typename T>
struct LaneSweep
{
   Launch L;
   int parts;
   mh::Args<T> A;
};
template <typename T>
mh_status plan_lane_sweep(mh_model *model, int64_t B, const mh_options &opts, const double *gravity, long slots, LaneSweep<T> &S)
{
   S.L = plan_launch(model->cu_count, B);
   S.parts = launch_parts(model->cu_count, S.L, std::min(8, model->n));
   if (const mh_status st = ensure_bytes(model->ws, lane_ws_bytes(slots, S.L, S.parts, sizeof(T))); st != MH_OK)
      return st;
   S.A = make_args<T>(model, B, opts, gravity);
   S.A.ws = (T *)model->ws.ptr;
   S.A.ws_stride = S.L.lanes;
   return MH_OK;
}
// the DoF indices no joint owns (the last row of the gravity gradient's zero table): entries the kernels fill with zeros
static void set_unowned(const mh_model *model, const int *&unowned, int &n_unowned)
{
   unowned = model->d_grav_zero_cols + model->grav_zero_ofs[model->n];
   n_unowned = model->grav_zero_ofs[model->n + 1] - model->grav_zero_ofs[model->n];
}

// A code object's launcher returns 0 when it launched, hipErrorNotSupported when the plan is not in the object (the caller goes on to
// its next plan) and anything else on failure.  True: the call is over, with status st.
bool spec_done(int rc, const char *what, mh_status &st)
{
   if (rc == (int)hipErrorNotSupported)
      return false;
   st = rc == 0 ? MH_OK : fail(MH_ERR_HIP, "%s: %s", what, hipGetErrorString((hipError_t)rc));
   return true;
}

// a kernel that takes more than 64 KB of dynamic LDS needs its limit raised, once per kernel and model
mh_status raise_lds_limit(mh_model *model, const void *kern, size_t lds)
{
   if (lds > 64 * 1024 && model->lds_attr[kern] < lds)
   {
      HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      model->lds_attr[kern] = lds;
   }
   return MH_OK;
}

// Big AoS batches of wide matrices go through transposed scratch copies (launch<T>; MH_GENERIC_TRANSPOSE forces the choice)
bool auto_transpose(const mh_model *m, int64_t B) { return B >= 8192 && m->nq + m->nv >= 64; }
bool transposes(const mh_model *m, int64_t B) { return m->use_transpose >= 0 ? m->use_transpose != 0 : auto_transpose(m, B); }

// tree-split kernels: 4 waves per 64 configurations; worth it while the batch cannot give every SIMD a wave of its own otherwise
// flags for the tree-split kernels: identity maps; rows staged in LDS when the layout is AoS, the maps are dense and it fits
int split_flags(const mh_model *m, int algo, bool soa)
{
   int flags = m->ident_maps ? SPEC_IDENT : 0;
   if (!soa && m->dense_maps && m->force_io != 0 && m->spec.split_lds_bytes(algo, SPEC_IO_LDS, m->nq, m->nv) <= 160 * 1024)
      flags |= SPEC_IO_LDS;
   return flags;
}
bool split_ok(const mh_model *m, int algo, int64_t B, bool soa)
{
   if (!m->spec.launch_split || !m->spec.split_usable || !m->spec.split_usable() || !m->use_spec || m->use_split == 0)
      return false;
   if (m->spec.split_lds_bytes(algo, split_flags(m, algo, soa), m->nq, m->nv) > 160 * 1024)
      return false;
   if (m->use_split == 1 || algo == 1 || algo == 0)
      return true; // ABA: the split form needs fewer registers; RNEA: two waves per SIMD and a trunk pass that is a fold of parked
                   // wrenches -- both measured faster than the whole-tree kernels at every batch size and in both layouts
   const long groups = groups_of(B);
   const long waves = groups * 4 * (algo == 2 ? 2 : 1);
   return waves <= (long)m->cu_count * 4 * kFusedFactor; // fused: while the batch cannot give every SIMD a wave of its own
}

// Bias-split forward dynamics (mh_zv_kernels.h): AoS matrices, dense index maps, every joint an effort source, no per-body outputs.
// The launch puts `jobs` workgroups of four waves on every 64 configurations, each with a CU's LDS nearly to itself: it pays while they
// all fit the device at once (measured, humanoid: pair 16.6 vs 18.3 us at B = 4096, 25.4 vs 19.3 at 8192; forward dynamics alone 17.0 vs
// 18.9 us at 8192, 31.2 vs 20.0 at 16384 -- profiles/r03_zv_vs_tree_split.txt); beyond that the tree-split kernels serve the call.
bool zv_ok(const mh_model *m, int64_t B, bool soa, int jobs)
{
   if (!m->spec.launch_zv || !m->spec.zv_usable || !m->spec.zv_usable() || !m->use_spec || !m->use_zv || m->use_split == 0)
      return false;
   if (soa || !m->dense_maps || m->force_io == 0 || m->n_locked > 0)
      return false;
   const long lds = m->spec.zv_lds_bytes(m->nq, m->nv);
   return lds > 0 && lds <= 160 * 1024 && (m->use_zv == 2 || groups_of(B) * jobs <= (long)m->cu_count);
}
// A wait of a bias-split launch that ran into its wall-clock limit (the producer workgroup never published): the kernel wrote NaN rows
// for that group and set the model's (context's) error word in mapped host memory.  It is a failure of an ASYNCHRONOUS call, so it is
// reported where the library next synchronises or is asked to: mh_model_check, mh_stream_synchronize, the *_host entry points after
// their own synchronisation, the create-time self-check -- and at the latest by the next bias-split call of the same model / context.
mh_status zv_check_error(mh_model *m)
{
   if (m->zv_error_host && *(volatile int *)m->zv_error_host != 0)
   {
      *(volatile int *)m->zv_error_host = 0;
      return fail(MH_ERR_HIP, "a bias-split forward dynamics launch gave up waiting for its bias rows (the accelerations of those configurations were written as NaN)");
   }
   return MH_OK;
}
mh_status check_all_error_words()
{
   std::lock_guard<std::mutex> lock(g_error_words_mutex);
   bool any = false;
   for (int *w : g_error_words)
      if (*(volatile int *)w != 0)
      {
         *(volatile int *)w = 0;
         any = true;
      }
   if (any)
      return fail(MH_ERR_HIP, "a bias-split forward dynamics launch gave up waiting for its bias rows (the accelerations of those configurations were written as NaN)");
   return MH_OK;
}
// scratch of the bias-split launches for batches up to B: the bias rows, the flags (zeroed on `stream`), the mapped error word
bool zv_self_signalling(const mh_model *m) { return m->ident_maps && m->spec.zv_self_signal && m->spec.zv_self_signal() != 0; }
mh_status zv_prepare(mh_model *m, int64_t B, hipStream_t stream)
{
   const size_t groups = (size_t)groups_of(B);
   mh_status st = ensure_bytes(m->zv_tau, groups * 64 * m->nv * sizeof(double)); // (whole groups: the two-stage hand-off keeps a matrix [nv][64] per group)
   if (st != MH_OK)
      return st;
   if (zv_self_signalling(m) && m->zv_cols.bytes < groups * 64 * m->nv * sizeof(double))
   { // the matrix whose limb columns signal themselves: sentinels wherever nothing has been published (filled ON THE LAUNCH STREAM, like the flags)
      st = ensure_bytes(m->zv_cols, std::max<size_t>(groups, 128) * 64 * m->nv * sizeof(double));
      if (st != MH_OK)
         return st;
      HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)m->zv_cols.ptr, 0x7ff4a5a5, m->zv_cols.bytes / 4, stream));
   }
   if (m->zv_flags.bytes < groups * mh::ZV_SYNC_STRIDE * sizeof(int))
   {
      st = ensure_bytes(m->zv_flags, std::max<size_t>(groups, 1024) * mh::ZV_SYNC_STRIDE * sizeof(int));
      if (st != MH_OK)
         return st;
      // zeroed ON THE LAUNCH STREAM: a plain hipMemset is not ordered against kernels of other streams (seen here as a rare refusal by the
      // create-time self-check: the memset landed after the bias job had stored its flag, and the inertia job ran into its time limit)
      HIP_TRY(hipMemsetAsync(m->zv_flags.ptr, 0, m->zv_flags.bytes, stream));
      m->zv_epoch = 0;
   }
   if (!m->zv_error_host)
   {
      HIP_TRY(hipHostMalloc((void **)&m->zv_error_host, 2 * sizeof(int), hipHostMallocMapped)); // [0] the error word, [1] the poison word's host copy
      m->zv_error_host[0] = m->zv_error_host[1] = 0;
      HIP_TRY(hipHostGetDevicePointer((void **)&m->zv_error_dev, m->zv_error_host, 0));
      std::lock_guard<std::mutex> lock(g_error_words_mutex);
      g_error_words.push_back(m->zv_error_host);
   }
   return MH_OK;
}
// jobs = 2: A.in3b = tau, A.outb = qdd.  jobs = 3: additionally A.in3 = qdd, A.out = tau.  done: the call is over (spec_done); false when
// the code object lacks the plan.
mh_status zv_launch(mh_model *m, mh::Args<double> &A, int jobs, hipStream_t stream, bool &done)
{
   done = false;
   mh_status st = zv_prepare(m, A.B, stream);
   if (st != MH_OK)
      return st;
   if (m->zv_epoch == 0x7fffffff)
   { // the flags have seen every positive value: start over
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemsetAsync(m->zv_flags.ptr, 0, m->zv_flags.bytes, stream));
      m->zv_epoch = 0;
   }
   const bool self_signal = zv_self_signalling(m);
   if (self_signal && *(volatile int *)(m->zv_error_host + 1) != 0)
   { // A consumer of this context gave up (mh_zv_kernels.h: zv_take_cols): its producer may have published AFTERWARDS, into a matrix nobody
     // reset -- every launch since has written NaN rows.  Wait for whatever is still running, sentinels everywhere, poison word cleared.
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)m->zv_cols.ptr, 0x7ff4a5a5, m->zv_cols.bytes / 4, stream));
      HIP_TRY(hipMemsetAsync(m->zv_flags.ptr, 0, m->zv_flags.bytes, stream));
      m->zv_epoch = 0;
      *(volatile int *)(m->zv_error_host + 1) = 0;
   }
   const int epoch = ++m->zv_epoch;
   int flags = SPEC_IO_LDS | (m->ident_maps ? SPEC_IDENT : 0);
   done = spec_done(m->spec.launch_zv(flags, &A, self_signal ? m->zv_cols.ptr : m->zv_tau.ptr, (int *)m->zv_flags.ptr, m->zv_error_dev, epoch, jobs,
                                      m->zv_same_l2, m->zv_wait_ticks, (void *)stream),
                    "bias-split kernel launch failed", st);
   return st;
}

// Forward dynamics of device-filling batches as two launches at two workgroups per CU (mh_zv_kernels.h, spec_zvb_*): the same calls the
// bias split serves (AoS matrices, dense index maps, every joint an effort source), taken from two groups of 64 configurations per CU
// upwards -- below that the one-job kernel gives every group a CU of its own and is faster (humanoid, one MI355X: 24.2 against 20.1 us
// at 16 384, 36.8 against 37.3 at 32 768, 64.9 against 73.1 at 65 536, 214.5 against 248.4 at 262 144: profiles/r04_zvb_vs_tree_split.txt).
bool zvb_ok(const mh_model *m, int64_t B, bool soa)
{
   if (!m->spec.launch_zvb || !m->spec.zvb_usable || !m->spec.zvb_usable() || !m->use_spec || !m->use_zvb || m->use_split == 0)
      return false;
   if (soa || !m->dense_maps || m->force_io == 0 || m->n_locked > 0)
      return false;
   return m->use_zvb == 2 || groups_of(B) >= 2 * (long)m->cu_count;
}
// ... and as ONE launch where the code object has the fused kernel (joints below the root all revolute / fixed, identity index maps)
bool zvf_ok(const mh_model *m, int64_t B, bool soa)
{
   if (!m->spec.launch_zvf || !m->spec.zvf_usable || !m->spec.zvf_usable() || !m->use_spec || !m->use_zvf || m->use_split == 0)
      return false;
   if (soa || !m->dense_maps || !m->ident_maps || m->force_io == 0 || m->n_locked > 0)
      return false;
   // measured (humanoid, one MI355X, profiles/r04_zvf_vs_others.txt): 20.5 us against the one-job kernel's 20.3 at 16 384 (one group per CU:
   // a tie), 27.0 against 36.4 at 24 576, 28.4 against 37.8 at 32 768, 195.9 against 250.5 at 262 144
   return m->use_zvf == 2 || groups_of(B) > (long)m->cu_count;
}
// Inverse dynamics of device-filling batches in a persistent loop that requests the next group's rows behind the trunk pass
// (spec_zvb_bias_kernel<.., BIAS = false>): AoS matrices, dense index maps; from three groups of 64 configurations per CU upwards, where
// every workgroup of the launch takes a second turn.  MH_RNEA_AHEAD=0: never, 2: whenever the call qualifies.
bool rnea_ahead_ok(const mh_model *m, int64_t B, bool soa)
{
   if (!m->spec.launch_rnea_ahead || !m->spec.zvb_usable || !m->spec.zvb_usable() || !m->use_spec || !m->use_rnea_ahead || m->use_split == 0)
      return false;
   if (soa || !m->dense_maps || m->force_io == 0)
      return false;
   return m->use_rnea_ahead == 2 || groups_of(B) > 2 * (long)m->cu_count;
}
mh_status zvb_launch(mh_model *m, mh::Args<double> &A, hipStream_t stream, bool &done)
{
   done = false;
   const size_t padded = (size_t)(groups_of(A.B) * 64);
   mh_status st = ensure_bytes(m->zv_tau, (size_t)A.B * m->nv * sizeof(double));
   if (st == MH_OK)
      st = ensure_bytes(m->zvb_cs, std::max<size_t>(1, (size_t)m->spec.zvb_cs_rows()) * padded * sizeof(double));
   if (st != MH_OK)
      return st;
   const int flags = SPEC_IO_LDS | (m->ident_maps ? SPEC_IDENT : 0);
   const long groups = std::min<long>(groups_of(A.B), (long)m->cu_count * 2);
   done = spec_done(m->spec.launch_zvb(flags, &A, m->zv_tau.ptr, m->zvb_cs.ptr, (long)padded, (int)groups, m->zvb_which, (void *)stream),
                    "two-launch forward dynamics failed to launch", st);
   return st;
}


// Depth-first run-time-topology kernels (mh_dfs_kernels.h): the frame plan of (algorithm, LDS budget) -- dfs_frames, mh_launch_plans.h --
// with its copy of the body records on the device.
const mh_model::DfsPlan *dfs_plan(mh_model *m, int algo, int budget)
{
   if (m->parent)
      m = m->parent; // the plans (device copies of the body records) belong to the model; its contexts share them
   std::lock_guard<std::mutex> lock(m->dfs_mutex);
   for (const mh_model::DfsPlan &p : m->dfs_plans)
      if (p.algo == algo && p.budget == budget)
         return &p;
   const FramePlan frames = dfs_frames(m->meta, m->n, algo, budget, m->dfs_place_greedy);
   mh_model::DfsPlan plan{algo, budget, frames.lds_slots, frames.glb_slots, frames.glb_frames, nullptr};
   if (hipMalloc((void **)&plan.d_meta, frames.meta.size() * sizeof(int)) != hipSuccess)
      return nullptr;
   if (hipMemcpy(plan.d_meta, frames.meta.data(), frames.meta.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
   {
      (void)hipFree(plan.d_meta);
      return nullptr;
   }
   m->dfs_plans.push_back(plan);
   return &m->dfs_plans.back();
}
void dfs_plans_drop(mh_model *m)
{
   std::lock_guard<std::mutex> lock(m->dfs_mutex);
   for (mh_model::DfsPlan &p : m->dfs_plans)
      (void)hipFree(p.d_meta);
   m->dfs_plans.clear();
}

// ---- run-time tree split (mh_split_kernels.h): the plan made at creation (split_rt_plan, split_rt_records: mh_launch_plans.h) and its
// device arrays, in upload order: one row each, walked by the upload and by the release (which reads the pointers only and passes no records)
std::vector<DeviceRow> split_rt_rows(mh_model *m, const SplitRecords *records = nullptr)
{
   mh_model::SplitRt &S = m->split_rt;
   static const SplitRecords none;
   std::vector<DeviceRow> rows = {device_row(S.d_trunk, S.trunk_list), device_row(S.d_seg, S.seg), device_row(S.d_xl_ofs, S.xl_ofs)};
   for (int k = 0; k < 3; k++)
   {
      const SplitRecords &r = records ? records[k] : none;
      rows.push_back(device_row(S.d_meta[k], r.meta));
      rows.push_back(device_row(S.d_xl[k], r.xl));
   }
   return rows;
}
void split_rt_free(mh_model *m)
{
   for (const DeviceRow &r : split_rt_rows(m))
      (void)hipFree(*r.ptr), *r.ptr = nullptr;
   m->split_rt.usable = false;
}
void split_rt_create(mh_model *m)
{
   mh_model::SplitRt &S = m->split_rt;
   static_cast<SplitPlan &>(S) = split_rt_plan(m->meta, m->n, m->n_slots);
   if (!S.usable)
      return;
   SplitRecords records[3];
   for (int k = 0; k < 3; k++)
      records[k] = split_rt_records(S, m->meta, m->n, k), S.lds_slots[k] = records[k].lds_slots;
   hipError_t e = hipSuccess;
   for (const DeviceRow &r : split_rt_rows(m, records))
   {
      if (e == hipSuccess)
         e = hipMalloc(r.ptr, r.bytes);
      if (e == hipSuccess)
         e = hipMemcpy(*r.ptr, r.host, r.bytes, hipMemcpyHostToDevice);
   }
   if (e != hipSuccess)
      split_rt_free(m);
}
// pair: both algorithms of mh_rnea_aba_f64 in ONE launch (mh::pair_split_kernel), for a model without a code object at small batches:
// A.in3 = qdd, A.out = tau, A.in3b = tau, A.outb = qdd.
template <typename T>
mh_status launch_split_rt(Algo algo, mh_model *model, int64_t B, mh::Args<T> &A, hipStream_t stream, bool pair = false)
{
   const mh_model::SplitRt &S = model->split_rt;
   const SplitShape shape = split_rt_shape(S.slots, S.lds_slots, model->cu_count, sizeof(T), algo, B, pair);
   const int k = shape.k, mode = shape.mode, grid = shape.grid;
   mh_status st = ensure_bytes(model->ws, split_rt_ws_bytes(S.slots, grid, sizeof(T)));
   if (st != MH_OK)
      return st;
   A.ws = (T *)model->ws.ptr;
   mh::SplitDev P{};
   P.meta = S.d_meta[k], P.trunk = S.d_trunk, P.seg = S.d_seg, P.xl_ofs = S.d_xl_ofs, P.xl = S.d_xl[k];
   P.n_trunk = S.n_trunk, P.slots = S.slots;
   for (int w = 0; w < mh::SPLIT_WAVES; w++)
      P.n_seg[w] = S.n_seg[w];
   const size_t lds = shape.lds;
#define MH_SPLIT_KERN(NAME) (mode == 0 ? (const void *)&mh::NAME<T, 0> : (mode == 1 ? (const void *)&mh::NAME<T, 1> : (const void *)&mh::NAME<T, 2>))
   const void *kern = algo == ALGO_RNEA ? MH_SPLIT_KERN(rnea_split_kernel) : (algo == ALGO_ABA ? MH_SPLIT_KERN(aba_split_kernel) : MH_SPLIT_KERN(crba_split_kernel));
   if constexpr (sizeof(T) == 8)
      if (pair || algo == ALGO_ABA)
      { // the single forward dynamics runs the pair call's machine code with one role: the two calls then agree bit for bit
         P.roles = pair ? 0 : 2;
         kern = MH_SPLIT_KERN(pair_split_kernel);
      }
#undef MH_SPLIT_KERN
   if ((st = raise_lds_limit(model, kern, lds)) != MH_OK)
      return st;
   void *args[] = {(void *)&A, (void *)&P};
   HIP_TRY(hipLaunchKernel(kern, dim3(grid), dim3(256), args, lds, stream));
   return MH_OK;
}

// Everything of a depth-first launch but the launch itself: the frame plan (uploaded at its first use), the grid, the global blocks
// behind it in model->ws and the kernel with its LDS attribute.  launch_dfs runs it for the call at hand, mh_reserve for every plan a
// batch up to its max_batch may get -- so that such a call finds all of it in place and only enqueues its kernel.
struct DfsSetup
{
   const mh_model::DfsPlan *plan;
   const void *kern;
   long lds, gslots;
   int grid;
   bool win;
};
// aos: the state rows are AoS (q_es == v_es == 1); pair: the fused RNEA + ABA walk (fp32 only)
template <typename T>
mh_status dfs_setup(Algo algo, mh_model *model, int64_t B, bool aos, bool pair, DfsSetup &S)
{
   const bool win = !pair && dfs_windows(*model, algo, sizeof(T), aos);
   const DfsChoice ch = dfs_choose(*model, *model, algo, sizeof(T), B, win, pair);
   const bool hand_lds = ch.hand_lds;
   const mh_model::DfsPlan *plan = dfs_plan(model, pair ? 2 : (algo == ALGO_RNEA ? 0 : 1), (int)ch.budget);
   if (!plan)
      return fail(MH_ERR_HIP, "depth-first kernels: the body records of the frame plan could not be uploaded");
   const DfsGeometry geo = dfs_geometry(ch, plan->lds_slots, plan->glb_slots, plan->glb_frames, groups_of(B), model->cu_count);
   const long lds = geo.lds, gslots = geo.gslots;
   const int grid = geo.grid, mode = geo.mode;
   mh_status st = ensure_bytes(model->ws, (size_t)gslots * (size_t)grid * 64 * sizeof(T));
   if (st != MH_OK)
      return st;
   const void *kern = nullptr;
   if (algo == ALGO_RNEA)
   {
      if (win)
         kern = mode == 0 ? (const void *)&mh::rnea_dfs_kernel<T, true, 0> : (mode == 1 ? (const void *)&mh::rnea_dfs_kernel<T, true, 1> : (const void *)&mh::rnea_dfs_kernel<T, true, 2>);
      else
         kern = mode == 0 ? (const void *)&mh::rnea_dfs_kernel<T, false, 0> : (mode == 1 ? (const void *)&mh::rnea_dfs_kernel<T, false, 1> : (const void *)&mh::rnea_dfs_kernel<T, false, 2>);
   }
   else if (pair)
   {
      if constexpr (sizeof(T) == 4)
      {
         if (hand_lds)
            kern = mode == 0 ? (const void *)&mh::aba_dfs_kernel<T, true, false, 0, true> : (const void *)&mh::aba_dfs_kernel<T, true, false, 2, true>;
         else
            kern = mode == 0 ? (const void *)&mh::aba_dfs_kernel<T, false, false, 0, true>
                             : (mode == 1 ? (const void *)&mh::aba_dfs_kernel<T, false, false, 1, true> : (const void *)&mh::aba_dfs_kernel<T, false, false, 2, true>);
      }
      else
         return fail(MH_ERR_INVALID_ARGUMENT, "the fused depth-first pair walk is built in fp32 only");
   }
   else if (ch.occ3 && sizeof(T) == 4)
   {
      if constexpr (sizeof(T) == 4)
      {
         if (hand_lds)
            kern = mode == 0 ? (const void *)&mh::aba_dfs_kernel<T, true, false, 0, false, true> : (const void *)&mh::aba_dfs_kernel<T, true, false, 2, false, true>;
         else
            kern = mode == 0 ? (const void *)&mh::aba_dfs_kernel<T, false, false, 0, false, true>
                             : (mode == 1 ? (const void *)&mh::aba_dfs_kernel<T, false, false, 1, false, true> : (const void *)&mh::aba_dfs_kernel<T, false, false, 2, false, true>);
      }
   }
   else if (hand_lds)
      kern = mode == 0 ? (const void *)&mh::aba_dfs_kernel<T, true, false, 0> : (const void *)&mh::aba_dfs_kernel<T, true, false, 2>;
   else
      kern = mode == 0 ? (const void *)&mh::aba_dfs_kernel<T, false, false, 0> : (mode == 1 ? (const void *)&mh::aba_dfs_kernel<T, false, false, 1> : (const void *)&mh::aba_dfs_kernel<T, false, false, 2>);
   if ((st = raise_lds_limit(model, kern, (size_t)lds)) != MH_OK)
      return st;
   S.plan = plan, S.kern = kern, S.lds = lds, S.gslots = gslots, S.grid = grid, S.win = win;
   return MH_OK;
}
// pair: the fused RNEA + ABA walk (aba_dfs_kernel<.., PAIR>; algo = ALGO_ABA, A.in3 = qdd, A.out = tau, A.in3b = tau in, A.outb = qdd out)
template <typename T>
mh_status launch_dfs(Algo algo, mh_model *model, int64_t B, mh::Args<T> &A, hipStream_t stream, bool pair = false)
{
   DfsSetup S{};
   const mh_status st = dfs_setup<T>(algo, model, B, A.q_es == 1 && A.v_es == 1, pair, S);
   if (st != MH_OK)
      return st;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = S.gslots * 64; // per-wave block of the global workspace: [grid][slots][64 lanes] -- the same constant slot stride as in LDS
   A.m.meta = S.plan->d_meta;
   if (algo == ALGO_RNEA)
      A.m.rnea_stack = S.plan->lds_slots;
   else
      A.m.aba_stack = S.plan->lds_slots;
   if (S.win)
      A.m.prog = model->d_prog_seq; // (the windows follow the matrices in engine order)
   void *args[] = {(void *)&A};
   HIP_TRY(hipLaunchKernel(S.kern, dim3(S.grid), dim3(64), args, (size_t)S.lds, stream));
   return MH_OK;
}

// What a call of launch<T> may ask for beyond one algorithm's plain output
template <typename T>
struct LaunchExtras
{
   const T *locked_in = nullptr; // forward dynamics with acceleration-source joints: their given accelerations ...
   T *locked_out = nullptr;      // ... and the efforts of all joints (may be NULL)
   T *body_acc = nullptr, *body_twist = nullptr; // per-body outputs (with bodies; either may be NULL)
   bool bodies = false;
   double dt = 0.0;                              // a simulation step of forward dynamics (mh_aba_integrate_f64): where a kernel can ride it
   T *q_next = nullptr, *qd_next = nullptr;      // along it writes the new state and sets *stepped
   bool *stepped = nullptr;
   T *joint_wrench = nullptr;                    // inverse dynamics with bodies: the wrench every joint transmits
};
// the simulation step riding in a forward-dynamics launch, and taking it off again when that plan is not in the code object
template <typename T>
void set_step(mh::Args<T> &A, const LaunchExtras<T> &x)
{
   A.dt = (T)x.dt, A.q_next = x.q_next, A.qd_next = x.qd_next;
}
template <typename T>
void clear_step(mh::Args<T> &A)
{
   A.dt = T(0), A.q_next = nullptr, A.qd_next = nullptr;
}

template <typename T>
mh_status launch(Algo algo, mh_model_t model, int64_t B, const T *q, const T *qd, const T *in3, const double gravity[3], const T *fext,
                 const mh_options *opts_in, T *out, const LaunchExtras<T> &x = LaunchExtras<T>())
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK; // an empty batch has nothing to read or write: NULL pointers are fine
   if (!q || !out || (algo != ALGO_CRBA && (!qd || !in3 || (!gravity && !opts.use_root_acceleration))))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   if (algo == ALGO_ABA && model->n_locked > 0 && !x.locked_in)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: forward dynamics needs their accelerations, use mh_aba_locked_f64",
                  model->n_locked);
   if (algo != ALGO_CRBA)
   { // the output may be qd, the third input, or q where nq == nv; the per-body / per-joint outputs are disjoint from everything
      const size_t bq = (size_t)B * model->nq * sizeof(T), bv = (size_t)B * model->nv * sizeof(T), bf = (size_t)B * model->n * 6 * sizeof(T);
      const InRange ins[4] = {{"q", q, bq}, {"qd", qd, bv}, {algo == ALGO_RNEA ? "qdd" : "tau", in3, bv}, {"f_ext", fext, bf}};
      const OutRange outs[4] = {{algo == ALGO_RNEA ? "tau_out" : "qdd_out", out, bv, model->q_may_be_out ? 7u : 6u}, {"body_acc_out", x.body_acc, bf, 0u},
                                {"body_twist_out", x.body_twist, bf, 0u}, {"joint_wrench_out", x.joint_wrench, bf, 0u}};
      if ((st = check_aliasing(algo == ALGO_RNEA ? "inverse dynamics" : "forward dynamics", ins, 4, outs, 4)) != MH_OK)
         return st;
   }
   // the sweep kernels' per-body workspace (plain RNEA / ABA calls run on the depth-first kernels, which size their own)
   // fp64 ABA stays on the sweep kernel: the depth-first walk fuses passes one and two, which in fp64 costs the whole register file plus
   // scratch (512 registers + 320 B against 310 and none) -- measured slower at every batch size on every 25..30-body model (humanoid
   // 112 vs 128 us at B = 4096, 1.04 vs 1.30 ms at 262144; profiles/r02_dfs_kernels_rates.txt).  In fp32 it fits and wins (config 5).
   const bool dfs_aba = sizeof(T) == 4 || model->dfs_place >= 0 || model->dfs_aba64;
   const bool dfs = model->use_dfs && algo != ALGO_CRBA && !x.bodies && !(algo == ALGO_ABA && (model->n_locked > 0 || !dfs_aba));
   if (!dfs)
   {
      st = ensure_workspace(model, B, sizeof(T));
      if (st != MH_OK)
         return st;
   }
   const Launch L = plan_launch(model->cu_count, B);
   hipStream_t stream = (hipStream_t)opts.stream;

   mh::Args<T> A = make_args<T>(model, B, opts, gravity);
   A.q = q, A.qd = qd, A.in3 = in3, A.fext = fext, A.out = out;
   A.body_acc = x.body_acc, A.body_twist = x.body_twist, A.joint_wrench = x.joint_wrench;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   const bool soa = opts.layout == MH_LAYOUT_SOA;

   if (x.bodies && algo != ALGO_CRBA)
   { // per-body outputs: run-time-topology kernels (the model's joint source modes must all be effort sources)
      if (model->n_locked > 0 && algo == ALGO_ABA)
         return fail(MH_ERR_INVALID_ARGUMENT, "per-body outputs of forward dynamics are not available while joints are acceleration sources");
      if (sizeof(T) == 8 && !x.joint_wrench && split_ok(model, algo == ALGO_RNEA ? 0 : 1, B, soa))
      { // the tree-split kernels write them too (identity maps, rows staged in LDS); other plans: the run-time-topology kernels below
         const int sf = split_flags(model, algo == ALGO_RNEA ? 0 : 1, soa);
         if ((sf & SPEC_IDENT) && (sf & SPEC_IO_LDS))
         {
            const long groups = std::min<long>(groups_of(B), (long)model->cu_count * 2);
            if (spec_done(model->spec.launch_split(algo == ALGO_RNEA ? 0 : 1, sf | SPEC_BODIES, &A, (int)groups, (void *)stream),
                          "tree-split kernel launch failed", st))
               return st;
         }
      }
      if (model->split_rt.usable && model->n_locked == 0 && (model->use_split_rt == 1 || groups_of(B) <= (long)model->cu_count * 2))
         return launch_split_rt<T>(algo, model, B, A, stream); // small batches: the run-time tree split writes the per-body outputs too
      if (algo == ALGO_RNEA)
         hipLaunchKernelGGL((mh::rnea_kernel<T, true>), dim3(L.grid), dim3(L.block), 0, stream, A);
      else
         hipLaunchKernelGGL((mh::aba_kernel<T, false, true>), dim3(L.grid), dim3(L.block), 0, stream, A);
      HIP_TRY(hipGetLastError());
      return MH_OK;
   }
   if (algo == ALGO_ABA && model->n_locked > 0)
   { // acceleration-source joints: run-time flags per joint, generic kernel only
      A.in3b = x.locked_in, A.outb = x.locked_out;
      hipLaunchKernelGGL((mh::aba_kernel<T, true>), dim3(L.grid), dim3(L.block), 0, stream, A);
      HIP_TRY(hipGetLastError());
      return MH_OK;
   }
   if constexpr (sizeof(T) == 8)
   {
      // (a simulation step rides in the inertia job where the index maps are the identity: the two-stage form of the hand-off integrates the
      // rows it holds and writes the new state too -- 17.5 against 20.1 us per step at B = 4096, profiles/r04_step_rates.txt)
      if (algo == ALGO_ABA && (!x.q_next || (model->ident_maps && model->use_zv_step)) && zv_ok(model, B, soa, 2))
      { // forward dynamics as two jobs side by side: bias efforts | articulated inertias, then the bias fold (mh_zv_kernels.h)
         if (const mh_status se = zv_check_error(model); se != MH_OK)
            return se;
         A.in3b = in3, A.outb = out;
         if (x.q_next)
            set_step(A, x);
         bool done = false;
         if ((st = zv_launch(model, A, 2, stream, done)) != MH_OK || done)
         {
            if (st == MH_OK && x.q_next && x.stepped)
               *x.stepped = true;
            return st;
         }
         A.in3b = nullptr, A.outb = nullptr; // not in this code object: the plans below
         clear_step(A);
      }
      if (algo == ALGO_ABA && (!x.q_next || model->use_zv_step) && zvf_ok(model, B, soa))
      { // device-filling batches: bias efforts, articulated inertias, fold and outward sweep of a group of 64 configurations by ONE workgroup
        // (a simulation step rides along: 32.3 against 42.4 us per step at 32 768, 226.5 against 286.7 at 262 144 -- profiles/r04_step_rates.txt)
         const long groups = std::min<long>(groups_of(B), (long)model->cu_count * 2);
         if (x.q_next)
            set_step(A, x);
         if (spec_done(model->spec.launch_zvf(SPEC_IO_LDS | SPEC_IDENT, &A, (int)groups, (void *)stream), "fused forward dynamics failed to launch", st))
         {
            if (st == MH_OK && x.q_next && x.stepped)
               *x.stepped = true;
            return st;
         }
         clear_step(A);
      }
      if (algo == ALGO_ABA && !x.q_next && zvb_ok(model, B, soa))
      { // ... or as two launches: bias rows and (cos, sin) pairs by one, articulated inertias + fold + outward sweep by the next
         bool done = false;
         if ((st = zvb_launch(model, A, stream, done)) != MH_OK || done)
            return st;
      }
   }
   if constexpr (sizeof(T) == 8)
   {
      if (algo == ALGO_RNEA && rnea_ahead_ok(model, B, soa))
      {
         const long groups = std::min<long>(groups_of(B), (long)model->cu_count * 2);
         if (spec_done(model->spec.launch_rnea_ahead(SPEC_IO_LDS | (model->ident_maps ? SPEC_IDENT : 0), &A, (int)groups, (void *)stream),
                       "inverse dynamics (rows requested ahead) failed to launch", st))
            return st;
      }
   }
   if (algo != ALGO_CRBA && sizeof(T) == 8 && split_ok(model, algo == ALGO_RNEA ? 0 : 1, B, soa))
   {
      int sf = split_flags(model, algo == ALGO_RNEA ? 0 : 1, soa);
      // device-filling RNEA batches without LDS rows (SoA): the build with a 168-register budget keeps three workgroups per CU busy
      // (124 -> 112 us at B = 262144); smaller batches are faster on the plain build
      const bool occ3 = algo == ALGO_RNEA && !(sf & SPEC_IO_LDS) && (sf & SPEC_IDENT) && groups_of(B) > (long)model->cu_count * 2;
      if (occ3)
         sf |= SPEC_OCC3;
      const long groups = std::min<long>(groups_of(B), (long)model->cu_count * (occ3 ? 3 : 2));
      if (algo == ALGO_ABA && x.q_next && (sf & SPEC_IDENT) && (sf & SPEC_IO_LDS))
      { // fused simulation step: the kernel integrates the rows it holds in LDS and writes the new state too
         set_step(A, x);
         if (x.stepped)
            *x.stepped = true;
      }
      if (spec_done(model->spec.launch_split(algo == ALGO_RNEA ? 0 : 1, sf, &A, (int)groups, (void *)stream), "tree-split kernel launch failed", st))
         return st;
      // a code object built without this plan (mh_build_code_object in its fast mode): the run-time-topology kernels serve the call
      clear_step(A);
      if (x.stepped)
         *x.stepped = false;
   }
   if (model->spec.launch && algo != ALGO_CRBA && model->use_spec && sizeof(T) == 8)
   {
      // Topology-specialised code object (fp64).  State rows are staged in LDS when the layout is AoS and they fit; ABA's
      // inward -> outward hand-over lives in LDS while the batch is small enough that one wave per CU is all the device
      // would get anyway, otherwise in the global workspace.
      const int a = algo == ALGO_RNEA ? 0 : 1;
      const long waves = groups_of(B);
      const long LDS_MAX = 160 * 1024;
      int flags = model->ident_maps ? SPEC_IDENT : 0;
      bool io = !soa && model->dense_maps && model->spec.supports(a, SPEC_IO_LDS) && model->spec.lds_bytes(a, SPEC_IO_LDS, model->nq, model->nv) <= LDS_MAX;
      if (model->force_io >= 0)
         io = io && model->force_io;
      if (io)
         flags |= SPEC_IO_LDS;
      if (algo == ALGO_ABA)
      {
         bool st = model->spec.lds_bytes(a, flags | SPEC_ST_LDS, model->nq, model->nv) <= LDS_MAX && waves <= (long)model->cu_count * kAbaLdsFactor;
         if (model->force_st >= 0)
            st = model->force_st && model->spec.lds_bytes(a, flags | SPEC_ST_LDS, model->nq, model->nv) <= LDS_MAX;
         if (st && !model->spec.supports(a, flags | SPEC_ST_LDS))
            flags &= ~SPEC_IO_LDS; // small batch: keep the hand-over in LDS, read the state rows directly
         if (st)
            flags |= SPEC_ST_LDS;
      }
      if (model->spec.supports(a, flags))
      {
      const long lds = model->spec.lds_bytes(a, flags, model->nq, model->nv);
      const long per_cu = lds > 0 ? std::max<long>(1, std::min<long>(8, LDS_MAX / lds)) : 8;
      const int grid = (int)std::max<long>(1, std::min(waves, (long)model->cu_count * per_cu));
      if (algo == ALGO_ABA && !(flags & SPEC_ST_LDS))
      {
         mh_status s2 = ensure_bytes(model->ws, (size_t)std::max(model->n_slots, model->spec.aba_slots()) * (size_t)grid * 64 * sizeof(T));
         if (s2 != MH_OK)
            return s2;
         A.ws = (T *)model->ws.ptr;
         A.ws_stride = (long)grid * 64;
      }
      if (spec_done(model->spec.launch(a, flags, &A, grid, (void *)stream), "specialised kernel launch failed", st))
         return st;
      A.ws = (T *)model->ws.ptr, A.ws_stride = L.lanes; // (a fast build without the whole-tree kernels: on to the run-time-topology kernels)
      } // else: this (algorithm, memory plan) is not in the code object -- the run-time-topology kernels below serve the call
   }
   // Small batches of a model whose tree branches: the tree split over the four waves of a workgroup (mh_split_kernels.h)
   if (model->split_rt.usable && algo != ALGO_CRBA && model->n_locked == 0 && !x.locked_in
       && (model->use_split_rt == 1 || groups_of(B) <= (long)model->cu_count * 2)) // measured: profiles/r02_split_rt_sweep.txt
      return launch_split_rt<T>(algo, model, B, A, stream);
   // Run-time-topology RNEA / ABA on AoS matrices: for big batches of wide matrices go through transposed scratch copies
   // (mh::transpose_kernel).  External wrenches keep their own strides.  The depth-first RNEA reads AoS rows through LDS windows instead
   // (mh_dfs_kernels.h, RowWindow); the depth-first ABA has no registers left for windows and takes the copies.
   T *t_out = nullptr;
   if (algo != ALGO_CRBA && !soa)
   {
      bool want = transposes(model, B);
      if (dfs && want)
         want = algo == ALGO_ABA || !model->ident_maps;
      if (want)
      {
         const size_t nq = model->nq, nv = model->nv;
         mh_status s3 = ensure_bytes(model->tr, (size_t)B * (nq + 3 * nv) * sizeof(T));
         if (s3 != MH_OK)
            return s3;
         T *t_q = (T *)model->tr.ptr, *t_qd = t_q + (size_t)B * nq, *t_in3 = t_qd + (size_t)B * nv;
         t_out = t_in3 + (size_t)B * nv;
         mh::transpose_rows<T>(q, t_q, (long)B, (long)nq, true, stream);
         mh::transpose_rows<T>(qd, t_qd, (long)B, (long)nv, true, stream);
         mh::transpose_rows<T>(in3, t_in3, (long)B, (long)nv, true, stream);
         A.q = t_q, A.qd = t_qd, A.in3 = t_in3, A.out = t_out;
         A.q_bs = 1, A.q_es = B, A.v_bs = 1, A.v_es = B;
      }
   }
   if (dfs)
   {
      st = launch_dfs<T>(algo, model, B, A, stream);
      if (st != MH_OK)
         return st;
   }
   else
   switch (algo)
   {
      case ALGO_RNEA:
         hipLaunchKernelGGL((mh::rnea_kernel<T>), dim3(L.grid), dim3(L.block), 0, stream, A);
         break;
      case ALGO_ABA:
         hipLaunchKernelGGL((mh::aba_kernel<T>), dim3(L.grid), dim3(L.block), 0, stream, A);
         break;
      case ALGO_CRBA:
      {
         const size_t hbytes = (size_t)B * model->nv * model->nv * sizeof(T);
         A.v_bs = soa ? 1 : (long)model->nv * model->nv;
         if (model->spec.launch_crba && model->spec.crba_packed && model->use_spec && sizeof(T) == 8)
         {
            const int sflags = (model->ident_maps && model->dense_maps) ? SPEC_IDENT : 0;
            // tree-split form (4 waves per 64 configurations, coalesced write-out): measured faster at every batch size
            bool split = sflags && !soa && model->spec.launch_crba_split && model->spec.crba_split_usable && model->spec.crba_split_usable()
                         && model->use_split != 0;
            if (split)
            {
               // thin workgroups (16 / 32 of the 64 lanes) while that is what it takes to give every CU a workgroup: the write-out is
               // bound by the stores one CU can have in flight
               // (the width that gives every CU exactly one: 16 at 4 096, 24 at 6 000 -- any width up to 64 runs)
               int lpg = (int)std::max<long>(16, std::min<long>(64, (B + model->cu_count - 1) / model->cu_count));
               if (const char *e = getenv("MH_CRBA_LPG"))
                  lpg = std::max(1, std::min(64, atoi(e)));
               const long ng = (B + lpg - 1) / lpg;
               if (spec_done(model->spec.launch_crba_split(&A, (int)std::min<long>(ng, (long)model->cu_count * 2), lpg, (void *)stream),
                             "tree-split CRBA launch failed", st))
                  return st;
            }
            const bool packed = model->spec.crba_packed(sflags) != 0;
            if (!packed)
               HIP_TRY(hipMemsetAsync(out, 0, hbytes, stream)); // direct-store kernel writes related entries only
            const int grid = packed ? (int)std::min<long>(groups_of(B), (long)model->cu_count) : L.grid;
            if (spec_done(model->spec.launch_crba(sflags, &A, grid, (void *)stream), "specialised CRBA launch failed", st))
               return st;
            // not in this code object (fast build): the run-time-topology kernels below
         }
         HIP_TRY(hipMemsetAsync(out, 0, hbytes, stream));
         if (model->split_rt.usable && (model->use_split_rt == 1 || groups_of(B) <= (long)model->cu_count * 2))
            return launch_split_rt<T>(algo, model, B, A, stream); // small batches: the tree split over four waves (mh_split_kernels.h)
         {
            const int parts = launch_parts(model->cu_count, L, std::min(8, model->n));
            if (const mh_status sp = ensure_bytes(model->ws, lane_ws_bytes(model->n_slots, L, parts, sizeof(T))); sp != MH_OK)
               return sp;
            A.ws = (T *)model->ws.ptr;
            hipLaunchKernelGGL((mh::crba_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, stream, A);
         }
         break;
      }
   }
   if (t_out)
   {
      mh::transpose_rows<T>((const T *)t_out, out, (long)B, (long)model->nv, false, stream);
   }
   HIP_TRY(hipGetLastError());
   return MH_OK;
}

// Two calls side by side: the second on the model's own stream, forked from and joined back into the caller's with events, on a
// workspace of its own -- every launch path sizes and reads model->ws, and model->tr (swap_tr) when it goes through transposed copies
// of the state matrices; then the first on the caller's stream.  Each call is given the options it is to run with.
template <class F1, class F2>
mh_status side_by_side(mh_model *model, const mh_options &opts, bool swap_tr, F1 first, F2 second)
{
   hipStream_t s = (hipStream_t)opts.stream;
   if (!model->pair_stream)
   {
      HIP_TRY(hipStreamCreateWithFlags(&model->pair_stream, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&model->pair_fork, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&model->pair_join, hipEventDisableTiming));
   }
   HIP_TRY(hipEventRecord(model->pair_fork, s));
   HIP_TRY(hipStreamWaitEvent(model->pair_stream, model->pair_fork, 0));
   mh_options ob = opts;
   ob.stream = (void *)model->pair_stream;
   std::swap(model->ws, model->ws_pair);
   if (swap_tr)
      std::swap(model->tr, model->tr_pair);
   const mh_status rb = second(&ob);
   std::swap(model->ws, model->ws_pair);
   if (swap_tr)
      std::swap(model->tr, model->tr_pair);
   const mh_status ra = first(&opts);
   HIP_TRY(hipEventRecord(model->pair_join, model->pair_stream)); // join even after an error: the caller's stream must not run ahead
   HIP_TRY(hipStreamWaitEvent(s, model->pair_join, 0));
   return rb != MH_OK ? rb : ra;
}
template <typename T>
LaunchExtras<T> body_outputs(T *body_acc, T *body_twist)
{
   LaunchExtras<T> x;
   x.body_acc = body_acc, x.body_twist = body_twist, x.bodies = true;
   return x;
}
LaunchExtras<double> joint_wrenches(double *joint_wrench)
{
   LaunchExtras<double> x;
   x.bodies = true, x.joint_wrench = joint_wrench;
   return x;
}
// Forward dynamics with acceleration-source joints (mh_aba_locked_*): tau_out gets the efforts of all joints
template <typename T>
mh_status aba_locked(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const T *qdd_in, const double gravity[3], const T *f_ext,
                     const mh_options *opts, T *qdd_out, T *tau_out)
{
   // the call's own validation first (launch<T> repeats it on the context's copy), then the aliasing rule, then any launch
   mh_options o;
   mh_status st0 = begin_call(model, B, opts, o);
   if (st0 != MH_OK)
      return st0;
   if (B > 0 && (!q || !qd || !tau || !qdd_out || (!gravity && !o.use_root_acceleration)))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   if (B > 0)
   { // qdd_out is qdd_in or apart from every input, tau_out is tau or apart from every input: the outward pass stores a joint's acceleration
     // and then copies its effort through, so qdd_out == tau would hand accelerations to tau_out
      const size_t bq = (size_t)B * model->nq * sizeof(T), bv = (size_t)B * model->nv * sizeof(T), bf = (size_t)B * model->n * 6 * sizeof(T);
      const InRange ins[5] = {{"q", q, bq}, {"qd", qd, bv}, {"tau", tau, bv}, {"qdd_in", qdd_in, bv}, {"f_ext", f_ext, bf}};
      const OutRange outs[2] = {{"qdd_out", qdd_out, bv, 1u << 3}, {"tau_out", tau_out, bv, 1u << 2}};
      if (const mh_status sa = check_aliasing("mh_aba_locked", ins, 5, outs, 2); sa != MH_OK)
         return sa;
   }
   if (model->n_locked == 0)
   { // nothing is locked: the ordinary forward dynamics, efforts copied through
      mh_status st = launch<T>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, &o, qdd_out);
      if (st == MH_OK && tau_out && tau_out != tau && B > 0)
         HIP_TRY(hipMemcpyAsync(tau_out, tau, (size_t)B * model->nv * sizeof(T), hipMemcpyDeviceToDevice, (hipStream_t)o.stream));
      return st;
   }
   if (B > 0 && !qdd_in)
      return fail(MH_ERR_INVALID_ARGUMENT, "qdd_in is NULL but %d joint(s) are acceleration sources", model->n_locked);
   LaunchExtras<T> x;
   x.locked_in = qdd_in, x.locked_out = tau_out;
   return launch<T>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, &o, qdd_out, x);
}

// Host-pointer front end (what a JNI / Panama shim with heap or off-heap arrays calls).  The batch is cut into chunks of rows that travel
// through a ring of three device slots on three streams: copy-in of chunk k+1, kernels of chunk k and copy-out of chunk k-1 overlap
// (PCIe is full duplex), kernels stay on ONE stream (they share the model's workspace).  The copies run at PCIe rate when the caller's
// matrices are pinned -- allocated with mh_host_alloc or registered with mh_host_register -- and at the runtime's staged rate otherwise.
// Returns when every output chunk has landed.  kind: ALGO_RNEA / ALGO_ABA / ALGO_CRBA, or PAIR: in3 = qdd, in4 = tau, out = tau_out,
// out2 = qdd_out (mh_rnea_aba_f64 per chunk).
enum
{
   HOST_PAIR = 100
};
mh_status host_pipeline_init(mh_model *m)
{
   if (m->hs_in)
      return MH_OK;
   HIP_TRY(hipStreamCreateWithFlags(&m->hs_in, hipStreamNonBlocking));
   HIP_TRY(hipStreamCreateWithFlags(&m->hs_run, hipStreamNonBlocking));
   HIP_TRY(hipStreamCreateWithFlags(&m->hs_out, hipStreamNonBlocking));
   for (int k = 0; k < 3; k++)
   {
      HIP_TRY(hipEventCreateWithFlags(&m->ev_in[k], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&m->ev_run[k], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&m->ev_out[k], hipEventDisableTiming));
   }
   return MH_OK;
}
template <typename T>
mh_status launch_host(int kind, mh_model_t model, int64_t B, const T *q, const T *qd, const T *in3, const T *in4, const double gravity[3],
                      const T *fext, const mh_options *opts_in, T *out, T *out2)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   const bool crba = kind == ALGO_CRBA, pair = kind == HOST_PAIR;
   if (!q || !out || (!crba && (!qd || !in3 || (!gravity && !opts.use_root_acceleration))) || (pair && (!in4 || !out2)))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   st = host_pipeline_init(model);
   if (st != MH_OK)
      return st;
   if (opts.stream)
      HIP_TRY(hipStreamSynchronize((hipStream_t)opts.stream)); // work the caller queued before this (synchronous) call
   const size_t nq = model->nq, nv = model->nv, nj = model->n;
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   // rows per chunk: SoA matrices are not cut (a chunk of configurations is not contiguous there); AoS: about an eighth of the batch,
   // 4096 .. 16384 configurations, whole waves
   // (measured, tools/host_path.py: a chunk costs ~60-80 us of copy / event calls, so a 4096-configuration batch is faster whole: 0.39 ms in
   // four chunks against 0.2 ms in one; from 16384 configurations on the overlap wins)
   int64_t chunk = B;
   if (!soa && model->host_chunk > 0 && B > model->host_chunk)
      chunk = std::max<int64_t>(64, ((int64_t)model->host_chunk + 63) / 64 * 64);
   else if (!soa && model->host_chunk == 0 && B >= 16384)
      chunk = std::max<int64_t>(4096, std::min<int64_t>(16384, (B / 8 + 63) / 64 * 64));
   const size_t c_q = (size_t)chunk * nq, c_v = (size_t)chunk * nv, c_f = fext ? (size_t)chunk * nj * 6 : 0;
   const size_t c_out = crba ? (size_t)chunk * nv * nv : c_v;
   const size_t slot = c_q + (crba ? 0 : 2 * c_v) + (pair ? c_v : 0) + c_f + c_out + (pair ? c_v : 0);
   const int64_t n_chunks = (B + chunk - 1) / chunk;
   const int ring = n_chunks > 1 ? 3 : 1;
   st = ensure_bytes(model->stage, slot * ring * sizeof(T));
   if (st != MH_OK)
      return st;
   mh_options o = opts;
   o.stream = (void *)model->hs_run;
   for (int64_t k = 0; k < n_chunks; k++)
   {
      const int s = (int)(k % ring);
      const int64_t r0 = k * chunk, rows = std::min<int64_t>(chunk, B - r0);
      T *d_q = (T *)model->stage.ptr + slot * s, *d_qd = d_q + c_q, *d_in3 = d_qd + (crba ? 0 : c_v), *d_in4 = d_in3 + (crba ? 0 : c_v);
      T *d_f = d_in4 + (pair ? c_v : 0), *d_out = d_f + c_f, *d_out2 = d_out + c_out;
      if (k >= ring)
         HIP_TRY(hipStreamWaitEvent(model->hs_in, model->ev_run[s], 0)); // the kernels of the slot's previous tenant have read their inputs
      const size_t b_q = (size_t)rows * nq * sizeof(T), b_v = (size_t)rows * nv * sizeof(T);
      HIP_TRY(hipMemcpyAsync(d_q, q + (size_t)r0 * nq, b_q, hipMemcpyHostToDevice, model->hs_in));
      if (!crba)
      {
         HIP_TRY(hipMemcpyAsync(d_qd, qd + (size_t)r0 * nv, b_v, hipMemcpyHostToDevice, model->hs_in));
         HIP_TRY(hipMemcpyAsync(d_in3, in3 + (size_t)r0 * nv, b_v, hipMemcpyHostToDevice, model->hs_in));
         if (pair)
            HIP_TRY(hipMemcpyAsync(d_in4, in4 + (size_t)r0 * nv, b_v, hipMemcpyHostToDevice, model->hs_in));
         if (fext)
            HIP_TRY(hipMemcpyAsync(d_f, fext + (size_t)r0 * nj * 6, (size_t)rows * nj * 6 * sizeof(T), hipMemcpyHostToDevice, model->hs_in));
      }
      HIP_TRY(hipEventRecord(model->ev_in[s], model->hs_in));
      HIP_TRY(hipStreamWaitEvent(model->hs_run, model->ev_in[s], 0));
      if (k >= ring)
         HIP_TRY(hipStreamWaitEvent(model->hs_run, model->ev_out[s], 0)); // ... and their outputs have left the slot
      if constexpr (sizeof(T) == 8)
      {
         if (pair)
            st = mh_rnea_aba_f64(model, rows, d_q, d_qd, d_in3, d_in4, gravity, fext ? d_f : nullptr, &o, d_out, d_out2);
         else
            st = launch<T>((Algo)kind, model, rows, d_q, d_qd, d_in3, gravity, fext ? d_f : nullptr, &o, d_out);
      }
      else
         st = launch<T>((Algo)kind, model, rows, d_q, d_qd, d_in3, gravity, fext ? d_f : nullptr, &o, d_out);
      if (st != MH_OK)
      {
         (void)hipDeviceSynchronize();
         return st;
      }
      HIP_TRY(hipEventRecord(model->ev_run[s], model->hs_run));
      HIP_TRY(hipStreamWaitEvent(model->hs_out, model->ev_run[s], 0));
      const size_t b_o = crba ? (size_t)rows * nv * nv * sizeof(T) : b_v;
      HIP_TRY(hipMemcpyAsync(out + (size_t)r0 * (crba ? nv * nv : nv), d_out, b_o, hipMemcpyDeviceToHost, model->hs_out));
      if (pair)
         HIP_TRY(hipMemcpyAsync(out2 + (size_t)r0 * nv, d_out2, b_v, hipMemcpyDeviceToHost, model->hs_out));
      HIP_TRY(hipEventRecord(model->ev_out[s], model->hs_out));
   }
   HIP_TRY(hipStreamSynchronize(model->hs_out));
   return zv_check_error(model); // before the caller reads the outputs
}
} // namespace

namespace
{
// Looks for libmecano_hip_topo_<key>.so next to this library and checks it was built for exactly this tree.
void try_load_spec(mh_model *m, const Plan &P)
{
   Dl_info info;
   if (!dladdr((const void *)&try_load_spec, &info) || !info.dli_fname)
      return;
   std::string dir(info.dli_fname);
   const size_t slash = dir.find_last_of('/');
   dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
   if (const char *e = getenv("MH_SPEC_DIR")) // experiment builds of the specialised code objects live elsewhere (tools/isa.py)
      dir = e;
   // the full code object, else a minimal one (mh_build_code_object's fast form: tree-split RNEA / ABA / pair for AoS + identity maps)
   std::string path = dir + "/libmecano_hip_topo_" + P.key + ".so";
   void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
   if (!h)
   {
      path = dir + "/libmecano_hip_topo_" + P.key + ".min.so";
      h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
   }
   if (!h)
      return;
   auto f_n = (int (*)(void))dlsym(h, "mh_spec_n");
   auto f_p = (const int *(*)(void))dlsym(h, "mh_spec_parents");
   auto f_t = (const int *(*)(void))dlsym(h, "mh_spec_types");
   SpecLib s;
   s.handle = h;
   s.launch = (decltype(s.launch))dlsym(h, "mh_spec_launch");
   s.lds_bytes = (decltype(s.lds_bytes))dlsym(h, "mh_spec_lds_bytes");
   s.aba_slots = (decltype(s.aba_slots))dlsym(h, "mh_spec_aba_slots");
   s.supports = (decltype(s.supports))dlsym(h, "mh_spec_supports");
   s.launch_fused = (decltype(s.launch_fused))dlsym(h, "mh_spec_launch_fused");
   s.fused_lds_bytes = (decltype(s.fused_lds_bytes))dlsym(h, "mh_spec_fused_lds_bytes");
   s.launch_crba = (decltype(s.launch_crba))dlsym(h, "mh_spec_launch_crba");
   s.crba_packed = (decltype(s.crba_packed))dlsym(h, "mh_spec_crba_packed");
   s.split_usable = (decltype(s.split_usable))dlsym(h, "mh_spec_split_usable");
   s.split_lds_bytes = (decltype(s.split_lds_bytes))dlsym(h, "mh_spec_split_lds_bytes");
   s.launch_split = (decltype(s.launch_split))dlsym(h, "mh_spec_launch_split");
   s.crba_split_usable = (decltype(s.crba_split_usable))dlsym(h, "mh_spec_crba_split_usable");
   s.launch_crba_split = (decltype(s.launch_crba_split))dlsym(h, "mh_spec_launch_crba_split");
   s.launch_rnea_crba = (decltype(s.launch_rnea_crba))dlsym(h, "mh_spec_launch_rnea_crba");
   s.zv_usable = (decltype(s.zv_usable))dlsym(h, "mh_spec_zv_usable");
   s.zv_lds_bytes = (decltype(s.zv_lds_bytes))dlsym(h, "mh_spec_zv_lds_bytes");
   s.launch_zv = (decltype(s.launch_zv))dlsym(h, "mh_spec_launch_zv");
   s.zv_self_signal = (decltype(s.zv_self_signal))dlsym(h, "mh_spec_zv_self_signal");
   s.zvb_usable = (decltype(s.zvb_usable))dlsym(h, "mh_spec_zvb_usable");
   s.zvb_cs_rows = (decltype(s.zvb_cs_rows))dlsym(h, "mh_spec_zvb_cs_rows");
   s.zvb_lds_bytes = (decltype(s.zvb_lds_bytes))dlsym(h, "mh_spec_zvb_lds_bytes");
   s.launch_zvb = (decltype(s.launch_zvb))dlsym(h, "mh_spec_launch_zvb");
   s.zvf_usable = (decltype(s.zvf_usable))dlsym(h, "mh_spec_zvf_usable");
   s.zvf_pair_usable = (decltype(s.zvf_pair_usable))dlsym(h, "mh_spec_zvf_pair_usable");
   s.launch_zvf = (decltype(s.launch_zvf))dlsym(h, "mh_spec_launch_zvf");
   s.launch_rnea_ahead = (decltype(s.launch_rnea_ahead))dlsym(h, "mh_spec_launch_rnea_ahead");
   s.rnea_crba_lds_bytes = (decltype(s.rnea_crba_lds_bytes))dlsym(h, "mh_spec_rnea_crba_lds_bytes");
   s.launch_coriolis = (decltype(s.launch_coriolis))dlsym(h, "mh_spec_launch_coriolis");
   s.launch_centroidal = (decltype(s.launch_centroidal))dlsym(h, "mh_spec_launch_centroidal");
   s.launch_coriolis_parts = (decltype(s.launch_coriolis_parts))dlsym(h, "mh_spec_launch_coriolis_parts");
   s.launch_centroidal_parts = (decltype(s.launch_centroidal_parts))dlsym(h, "mh_spec_launch_centroidal_parts");
   s.abi = (decltype(s.abi))dlsym(h, "mh_spec_abi");
   // the code object reinterprets the library's argument structs and folds parts of the canonical-frame convention at compile time:
   // it must have been built from the same headers (a stale or foreign libmecano_hip_topo_<key>.so is refused, visibly)
   if (!s.abi || s.abi() != mh::spec_abi_stamp())
   {
      char note[256];
      snprintf(note, sizeof note, "generic (code object %s refused: built against another library version, ABI stamp %016llx, this library %016llx)",
               path.c_str(), s.abi ? s.abi() : 0ull, mh::spec_abi_stamp());
      m->variant = note;
      dlclose(h);
      return;
   }
   // ... and from the same KERNEL sources and code-generation flags as the ones this library was built beside: a code object left over
   // from an experiment or an older tree computes something, passes its own self-check against nothing but itself, and is not HEAD's
   s.sources_hash = (decltype(s.sources_hash))dlsym(h, "mh_spec_sources_hash");
   if (!s.sources_hash || strcmp(s.sources_hash(), MH_STR_(MH_SPEC_SOURCES_HASH)) != 0)
   {
      char note[320];
      snprintf(note, sizeof note, "generic (code object %s refused: built from other kernel sources or flags, source hash %s, this library expects %s)",
               path.c_str(), s.sources_hash ? s.sources_hash() : "(none)", MH_STR_(MH_SPEC_SOURCES_HASH));
      m->variant = note;
      dlclose(h);
      return;
   }
   bool ok = f_n && f_p && f_t && s.launch && s.lds_bytes && s.aba_slots && s.supports && f_n() == m->n;
   for (int e = 0; ok && e < m->n; e++)
      ok = f_p()[e] == P.eparent[e] && f_t()[e] == P.etype[e];
   if (!ok)
   {
      m->variant = "generic (code object " + path + " refused: it was built for another tree)";
      dlclose(h);
      return;
   }
   m->spec = s;
   m->variant = "topo:" + P.key;
   auto f_min = (int (*)(void))dlsym(h, "mh_spec_minimal");
   m->spec_minimal = f_min && f_min() != 0;
   if (m->spec_minimal)
      m->variant += " (minimal build: tree-split RNEA / ABA / pair kernels only, every other plan on the run-time-topology kernels)";
}
// Mass matrix + Coriolis matrix (CompositeRigidBodyMassMatrixCalculator with the Coriolis calculation enabled): run-time-topology kernel
template <typename T>
mh_status coriolis_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const mh_options *opts_in, T *H_out, T *C_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !H_out || !C_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   const Launch L = plan_launch(model->cu_count, B);
   const int parts = launch_parts(model->cu_count, L, std::min(8, model->n));
   st = ensure_bytes(model->ws, lane_ws_bytes(model->n_slots, L, parts, sizeof(T)));
   if (st != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   mh::Args<T> A = make_args<T>(model, B, opts);
   A.q = q, A.qd = qd, A.out = H_out, A.outb = C_out;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   set_strides(A.f_bs, A.f_es, opts.layout == MH_LAYOUT_SOA, B, (long)model->nv * model->nv); // strides of H and C
   const size_t hbytes = (size_t)B * model->nv * model->nv * sizeof(T);
   HIP_TRY(hipMemsetAsync(H_out, 0, hbytes, stream)); // the kernel writes the entries of related joints only (:298-300)
   HIP_TRY(hipMemsetAsync(C_out, 0, hbytes, stream));
   if constexpr (sizeof(T) == 8)
   {
      if (model->spec.launch_coriolis && model->use_spec)
      { // topology-specialised recursion: ancestors' transforms and velocities in registers, no workspace
         const int grid = (int)std::max<long>(1, std::min(groups_of(B), (long)model->cu_count * 4));
         Launch G = L;
         G.grid = grid; // small batches: several waves per group of configurations, each writing every parts-th body's columns
         const int rc = model->spec.launch_coriolis_parts
                           ? model->spec.launch_coriolis_parts(model->ident_maps ? SPEC_IDENT : 0, &A, grid, launch_parts(model->cu_count, G, std::min(8, model->n)), (void *)stream)
                           : model->spec.launch_coriolis(model->ident_maps ? SPEC_IDENT : 0, &A, grid, (void *)stream);
         if (spec_done(rc, "specialised Coriolis kernel launch failed", st))
            return st;
      }
   }
   hipLaunchKernelGGL((mh::coriolis_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, stream, A);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Joint torque regressor (JointTorqueRegressorCalculator): run-time-topology kernel
template <typename T>
mh_status regressor_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const double *gravity, const mh_options *opts_in,
                         int32_t first_moment_columns, T *Y_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !qdd || !Y_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   LaneSweep<T> S;
   if ((st = plan_lane_sweep<T>(model, B, opts, gravity, model->n_slots, S)) != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   mh::Args<T> &A = S.A;
   A.q = q, A.qd = qd, A.in3 = qdd, A.out = Y_out;
   const long ysize = (long)model->nv * model->n * 10;
   set_strides(A.f_bs, A.f_es, opts.layout == MH_LAYOUT_SOA, B, ysize); // strides of Y
   // entries of joints that do not support a body are zero, and so are the reference's centre-of-mass columns (mh_kernels.h)
   HIP_TRY(hipMemsetAsync(Y_out, 0, (size_t)B * ysize * sizeof(T), stream));
   // the centre-of-mass columns: d tau / d (m c) on request; else the reference's -- zero, or e x a once the twist is switched off
   const int mode = first_moment_columns ? 1 : (opts.consider_coriolis ? 0 : 2);
   if (mode == 0)
      hipLaunchKernelGGL((mh::regressor_kernel<T, 0>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, stream, A);
   else if (mode == 1)
      hipLaunchKernelGGL((mh::regressor_kernel<T, 1>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, stream, A);
   else
      hipLaunchKernelGGL((mh::regressor_kernel<T, 2>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, stream, A);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status centroidal_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const double *frame, int32_t frame_mode, const mh_options *opts_in,
                          T *A_out, T *b_out, T *com_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (frame_mode != MH_CENTROIDAL_FRAME_FIXED && frame_mode != MH_CENTROIDAL_FRAME_AT_COM)
      return fail(MH_ERR_INVALID_ARGUMENT, "unknown centroidal frame mode %d", frame_mode);
   if (B == 0)
      return MH_OK;
   if (!q || !A_out || (b_out && !qd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer (the convective term needs qd)");
   const Launch L = plan_launch(model->cu_count, B);
   const int parts = launch_parts(model->cu_count, L, std::min(8, model->n));
   st = ensure_bytes(model->ws, lane_ws_bytes(model->n_slots, L, parts, sizeof(T)));
   if (st != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   mh::CentArgs<T> A{};
   A.m = dev_model<T>(model);
   A.B = B;
   A.q = q, A.qd = qd, A.A = A_out, A.b = b_out, A.com = com_out;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   set_strides(A.q_bs, A.q_es, soa, B, model->nq);
   set_strides(A.v_bs, A.v_es, soa, B, model->nv);
   set_strides(A.a_bs, A.a_es, soa, B, 6L * model->nv);
   set_strides(A.b_bs, A.b_es, soa, B, 6);
   set_strides(A.c_bs, A.c_es, soa, B, 3);
   for (int k = 0; k < 9; k++)
      A.fR[k] = frame ? (T)frame[k] : (T)(k % 4 == 0 ? 1 : 0);
   for (int k = 0; k < 3; k++)
      A.fp[k] = frame ? (T)frame[9 + k] : T(0);
   A.at_com = frame_mode == MH_CENTROIDAL_FRAME_AT_COM;
   HIP_TRY(hipMemsetAsync(A_out, 0, (size_t)B * 6 * model->nv * sizeof(T), stream)); // columns no considered joint owns stay zero
   if constexpr (sizeof(T) == 8)
   {
      if (model->spec.launch_centroidal && model->use_spec)
      {
         const int grid = (int)std::max<long>(1, std::min(groups_of(B), (long)model->cu_count * 4));
         Launch G = L;
         G.grid = grid;
         const int rc = model->spec.launch_centroidal_parts
                           ? model->spec.launch_centroidal_parts(model->ident_maps ? SPEC_IDENT : 0, &A, grid, launch_parts(model->cu_count, G, std::min(8, model->n)), (void *)stream)
                           : model->spec.launch_centroidal(model->ident_maps ? SPEC_IDENT : 0, &A, grid, (void *)stream);
         if (spec_done(rc, "specialised centroidal kernel launch failed", st))
            return st;
      }
   }
   hipLaunchKernelGGL((mh::centroidal_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, stream, A);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Gravity efforts and their gradient (MultiBodyGravityGradientCalculator): run-time-topology kernel, which writes every entry of its
// outputs -- no memset in front of it
template <typename T>
mh_status gravity_gradient_impl(mh_model_t model, int64_t B, const T *q, const double *gravity, const T *f_ext, const mh_options *opts_in, T *tau_out,
                                T *grad_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (!gravity)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL");
   if (!tau_out && !grad_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "tau_out and grad_out are both NULL");
   if (B == 0)
      return MH_OK;
   if (!q)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL configuration pointer");
   const Launch L = plan_launch(model->cu_count, B);
   const int parts = launch_parts(model->cu_count, L, std::min(8, model->n));
   st = ensure_bytes(model->ws, lane_ws_bytes(model->n_slots, L, parts, sizeof(T)));
   if (st != MH_OK)
      return st;
   mh::GravArgs<T> G{};
   mh::Args<T> &A = G.a;
   A = make_args<T>(model, B, opts);
   A.q = q, A.fext = f_ext, A.out = tau_out, A.outb = grad_out;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   A.gx = (T)gravity[0], A.gy = (T)gravity[1], A.gz = (T)gravity[2]; // the vector itself: opts->root_acceleration plays no part
   set_strides(G.g_bs, G.g_es, opts.layout == MH_LAYOUT_SOA, B, (long)model->nv * model->nv);
   G.sub_mass = sizeof(T) == 8 ? (const T *)model->d_sub_mass64 : (const T *)model->d_sub_mass32;
   G.zero_ofs = model->d_grav_zero_ofs, G.zero_cols = model->d_grav_zero_cols;
   hipLaunchKernelGGL((mh::gravity_gradient_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Inverse apparent inertia of K target bodies (MultiBodyResponseCalculator): run-time-topology kernel, which writes every entry of W --
// no memset in front of it.  Targets and their frames travel as kernel arguments; which bodies the sweeps visit is decided on the device
// from the model's Euler tour, so the call uploads nothing and allocates nothing beyond the workspace mh_reserve covers.
// The launch: targets in range with their canonical frames (target_frame), opts resolved to its context (begin_call).
// w_soa: W goes out as [entries][B] whatever the call's layout (scratch of the constrained dynamics)
template <typename T>
mh_status apparent_inertia_launch(mh_model *model, int64_t B, const T *q, int n_targets, const int32_t *joints, const double (*canon)[12], bool coupled,
                                  const mh_options &opts, T *W_out, bool w_soa)
{
   const Launch L = plan_launch(model->cu_count, B);
   const int parts = launch_parts(model->cu_count, L, n_targets);
   if (mh_status st = ensure_bytes(model->ws, lane_ws_bytes(model->resp_slots, L, parts, sizeof(T))); st != MH_OK)
      return st;
   mh::RespArgs<T> G{};
   for (int k = 0; k < n_targets; k++)
   {
      G.tgt[k] = model->engine_of[joints[k]];
      for (int r = 0; r < 12; r++)
         G.pose[k][r] = (T)canon[k][r];
   }
   mh::Args<T> &A = G.a;
   A = make_args<T>(model, B, opts);
   A.q = q, A.out = W_out;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   set_strides(G.w_bs, G.w_es, w_soa || opts.layout == MH_LAYOUT_SOA, B, 36L * n_targets * (coupled ? n_targets : 1));
   G.info = model->d_resp_info;
   G.slots = model->resp_slots, G.a_base = model->resp_a_base, G.u_base = model->resp_u_base;
   G.n_targets = n_targets, G.coupled = coupled;
   hipLaunchKernelGGL((mh::apparent_inertia_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status apparent_inertia_impl(mh_model_t model, int64_t B, const T *q, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                int32_t blocks, const mh_options *opts_in, T *W_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (n_targets < 1 || n_targets > MH_MAX_APPARENT_TARGETS)
      return fail(MH_ERR_INVALID_ARGUMENT, "n_targets = %d is outside 1 ... %d", n_targets, MH_MAX_APPARENT_TARGETS);
   if (blocks != MH_APPARENT_BLOCKS_DIAGONAL && blocks != MH_APPARENT_BLOCKS_COUPLED)
      return fail(MH_ERR_INVALID_ARGUMENT, "unknown blocks value %d", blocks);
   if (!target_joints)
      return fail(MH_ERR_INVALID_ARGUMENT, "target_joints is NULL");
   double canon[MH_MAX_APPARENT_TARGETS][12];
   for (int k = 0; k < n_targets; k++)
   {
      const int i = target_joints[k];
      if (i < 0 || i >= model->n)
         return fail(MH_ERR_INVALID_ARGUMENT, "target %d names joint %d (the model has %d joints)", k, i, model->n);
      if ((st = target_frame<double>(model, model->engine_of[i], target_poses ? target_poses + 12 * k : nullptr, canon[k], nullptr, k)) != MH_OK)
         return st;
   }
   if (B == 0)
      return MH_OK;
   if (!q || !W_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL configuration / output pointer");
   const bool coupled = blocks == MH_APPARENT_BLOCKS_COUPLED;
   {
      const InRange in{"q", q, (size_t)B * model->nq * sizeof(T)};
      const OutRange out{"W_out", W_out, (size_t)B * 36 * n_targets * (coupled ? n_targets : 1) * sizeof(T), 0u};
      if ((st = check_aliasing("mh_apparent_inertia_inverse", &in, 1, &out, 1)) != MH_OK)
         return st;
   }
   return apparent_inertia_launch<T>(model, B, q, n_targets, target_joints, canon, coupled, opts, W_out, false);
}
// Poses of frames fixed in bodies and geometric Jacobians between bodies (mh_kinematics_kernels.h): run-time-topology kernels, which write
// every entry of their outputs -- no memset in front of them.  Targets, bases and frames travel as kernel arguments.  The kernels store
// SoA (coalesced) always: AoS outputs are produced in scratch of the context and brought to rows by a transposition, so that no lane
// writes entries 6 K nv elements apart.
static size_t kin_scratch_entries(const mh_model *m, int n_targets, bool jacobian, bool conv)
{
   return jacobian ? 6 * (size_t)n_targets * (size_t)m->nv + (conv ? 6 * (size_t)n_targets : 0) : 12 * (size_t)n_targets;
}
// The target list of a kinematics call, forward or reverse: counts and indices checked, targets and bases as engine indices, each target
// frame in the canonical frame of its body (target_frame).  with_all_bodies: target_joints = NULL names every body (all_bodies is set).
template <typename T>
mh_status kin_targets(const char *call, bool with_all_bodies, mh_model_t model, int32_t n_targets, const int32_t *base_joints,
                      const int32_t *target_joints, const double *target_poses, int *tgt, int *base, T (*pose)[12], bool &all_bodies)
{
   mh_status st = MH_OK;
   all_bodies = with_all_bodies && !target_joints;
   if (all_bodies)
   {
      if (n_targets != model->n)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target_joints is NULL (every body) but n_targets = %d is not the model's %d joints", call, n_targets, model->n);
      if (target_poses)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target_poses given without target_joints (every body comes with the identity pose)", call);
   }
   else
   {
      if (!target_joints)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target_joints is NULL", call);
      if (n_targets < 1 || n_targets > MH_MAX_KINEMATIC_TARGETS)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: n_targets = %d is outside 1 ... %d", call, n_targets, MH_MAX_KINEMATIC_TARGETS);
   }
   for (int k = 0; k < (all_bodies ? 0 : n_targets); k++)
   {
      const int i = target_joints[k], ib = base_joints ? base_joints[k] : -1;
      if (i < -1 || i >= model->n)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d names joint %d (the model has %d joints; -1 is the root body)", call, k, i, model->n);
      if (ib < -1 || ib >= model->n)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: base %d names joint %d (the model has %d joints; -1 is the root body)", call, k, ib, model->n);
      tgt[k] = i < 0 ? -1 : model->engine_of[i];
      base[k] = ib < 0 ? -1 : model->engine_of[ib];
      if ((st = target_frame<T>(model, tgt[k], target_poses ? target_poses + 12 * k : nullptr, pose[k], call, k)) != MH_OK)
         return st;
   }
   return MH_OK;
}
template <typename T>
mh_status kinematics_impl(const char *call, bool jacobian, mh_model_t model, int64_t B, const T *q, const T *qd, int32_t n_targets,
                          const int32_t *base_joints, const int32_t *target_joints, const double *target_poses, const mh_options *opts_in,
                          T *pose_out, T *J_out, T *conv_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   mh::KinArgs<T> G{};
   bool all_bodies = false;
   if ((st = kin_targets<T>(call, !jacobian, model, n_targets, base_joints, target_joints, target_poses, G.tgt, G.base, G.pose, all_bodies)) != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || (jacobian ? !J_out : !pose_out))
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: NULL configuration / output pointer", call);
   if (conv_out && !qd)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: the convective term needs qd", call);
   const size_t n_pose = 12 * (size_t)n_targets, n_J = 6 * (size_t)n_targets * (size_t)model->nv, n_conv = 6 * (size_t)n_targets;
   {
      const size_t bq = (size_t)B * model->nq * sizeof(T), bv = (size_t)B * model->nv * sizeof(T);
      const InRange ins[2] = {{"q", q, bq}, {"qd", jacobian ? qd : nullptr, bv}};
      const OutRange outs[3] = {{"pose_out", pose_out, (size_t)B * n_pose * sizeof(T), 0u},
                                {"J_out", J_out, (size_t)B * n_J * sizeof(T), 0u},
                                {"conv_out", conv_out, (size_t)B * n_conv * sizeof(T), 0u}};
      if ((st = check_aliasing(call, ins, 2, outs, 3)) != MH_OK)
         return st;
   }
   const Launch L = plan_launch(model->cu_count, B);
   const int parts = jacobian ? launch_parts(model->cu_count, L, n_targets) : 1;
   st = ensure_bytes(model->ws, lane_ws_bytes((long)model->n * mh::KIN_SLOTS, L, parts, sizeof(T)));
   if (st != MH_OK)
      return st;
   // B = 1: the two layouts are the same memory
   const bool staged = opts.layout != MH_LAYOUT_SOA && B > 1;
   T *pose_dst = pose_out, *J_dst = J_out, *conv_dst = conv_out;
   if (staged)
   {
      st = ensure_bytes(model->kin, (size_t)B * kin_scratch_entries(model, n_targets, jacobian, conv_out != nullptr) * sizeof(T));
      if (st != MH_OK)
         return st;
      pose_dst = J_dst = (T *)model->kin.ptr;
      if (conv_out)
         conv_dst = J_dst + (size_t)B * n_J;
   }
   hipStream_t stream = (hipStream_t)opts.stream;
   mh::Args<T> &A = G.a;
   A = make_args<T>(model, B, opts);
   A.q = q, A.qd = conv_out ? qd : nullptr;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   G.pose_out = pose_dst, G.J = J_dst, G.conv = conv_dst;
   G.p_bs = G.j_bs = G.c_bs = 1, G.p_es = G.j_es = G.c_es = (long)B;
   G.info = model->d_resp_info;
   G.zero_ofs = model->d_grav_zero_ofs, G.zero_cols = model->d_grav_zero_cols;
   G.n_targets = n_targets, G.all_bodies = all_bodies;
   if (jacobian)
      hipLaunchKernelGGL((mh::geometric_jacobian_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, stream, G);
   else
      hipLaunchKernelGGL((mh::body_poses_kernel<T>), dim3(L.grid), dim3(L.block), 0, stream, G);
   HIP_TRY(hipGetLastError());
   if (staged)
   {
      if (!jacobian)
         mh::transpose_rows<T>(pose_dst, pose_out, (long)B, (long)n_pose, false, stream);
      else
      {
         if (n_J)
            mh::transpose_rows<T>(J_dst, J_out, (long)B, (long)n_J, false, stream);
         if (conv_out)
            mh::transpose_rows<T>(conv_dst, conv_out, (long)B, (long)n_conv, false, stream);
      }
      HIP_TRY(hipGetLastError());
   }
   return MH_OK;
}
// Reverse mode of the kinematics (mh_kinematics_vjp_kernels.h): the gradient of a loss on body poses with respect to q (g = the cotangent
// of pose_out, 12 per target) and, wrench = true, J^T w of up to sixteen chains (g = the wrenches, 6 per target).  One kernel in the
// workspace plan of the forward calls (parts = 1), which reads and writes SoA always: an AoS batch has its cotangents transposed into the
// context's kin scratch, the kernel writes the nv entries behind them, and a second transposition brings those to the caller's rows.
static size_t kin_vjp_scratch_entries(const mh_model *m, int n_targets, bool wrench) { return (wrench ? 6 : 12) * (size_t)n_targets + (size_t)m->nv; }
template <typename T>
mh_status kinematics_vjp_impl(const char *call, bool wrench, mh_model_t model, int64_t B, const T *q, int32_t n_targets, const int32_t *base_joints,
                              const int32_t *target_joints, const double *target_poses, const T *g, const mh_options *opts_in, T *out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   mh::KinVjpArgs<T> G{};
   bool all_bodies = false;
   if ((st = kin_targets<T>(call, !wrench, model, n_targets, base_joints, target_joints, target_poses, G.tgt, G.base, G.pose, all_bodies)) != MH_OK)
      return st;
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !g || !out)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: NULL configuration / %s / output pointer", call, wrench ? "wrench" : "cotangent");
   const size_t n_g = (wrench ? 6 : 12) * (size_t)n_targets, nv = (size_t)model->nv;
   {
      const InRange ins[2] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {wrench ? "wrench" : "g_pose", g, (size_t)B * n_g * sizeof(T)}};
      const OutRange outs[1] = {{wrench ? "tau_out" : "gq_out", out, (size_t)B * nv * sizeof(T), 0u}};
      if ((st = check_aliasing(call, ins, 2, outs, 1)) != MH_OK)
         return st;
   }
   const Launch L = plan_launch(model->cu_count, B);
   st = ensure_bytes(model->ws, lane_ws_bytes((long)model->n * mh::KIN_SLOTS, L, 1, sizeof(T)));
   if (st != MH_OK)
      return st;
   // B = 1: the two layouts are the same memory
   const bool staged = opts.layout != MH_LAYOUT_SOA && B > 1;
   const T *g_src = g;
   T *out_dst = out;
   hipStream_t stream = (hipStream_t)opts.stream;
   if (staged)
   {
      st = ensure_bytes(model->kin, (size_t)B * kin_vjp_scratch_entries(model, n_targets, wrench) * sizeof(T));
      if (st != MH_OK)
         return st;
      T *t_g = (T *)model->kin.ptr;
      mh::transpose_rows<T>(g, t_g, (long)B, (long)n_g, true, stream);
      HIP_TRY(hipGetLastError());
      g_src = t_g, out_dst = t_g + (size_t)B * n_g;
   }
   mh::Args<T> &A = G.a;
   A = make_args<T>(model, B, opts);
   A.q = q;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   G.g = g_src, G.out = out_dst;
   G.g_bs = G.o_bs = 1, G.g_es = G.o_es = (long)B;
   G.info = model->d_resp_info;
   G.zero_ofs = model->d_grav_zero_ofs, G.zero_cols = model->d_grav_zero_cols;
   G.n_targets = n_targets, G.all_bodies = all_bodies;
   if (wrench)
      hipLaunchKernelGGL((mh::kinematics_vjp_kernel<T, true>), dim3(L.grid), dim3(L.block), 0, stream, G);
   else
      hipLaunchKernelGGL((mh::kinematics_vjp_kernel<T, false>), dim3(L.grid), dim3(L.block), 0, stream, G);
   HIP_TRY(hipGetLastError());
   if (staged)
   {
      mh::transpose_rows<T>(out_dst, out, (long)B, (long)nv, false, stream);
      HIP_TRY(hipGetLastError());
   }
   return MH_OK;
}
// Forward dynamics under bilateral constraints on body frames, its velocity-level twin (mh_constraint_kernels.h) and the frictional contact
// impulses (mh_contact_kernels.h): launches composed on the caller's stream -- the free forward dynamics with per-body accelerations
// (velocity level: the inverse dynamics with per-body twists), the COUPLED inverse apparent inertia at the call's frames into SoA scratch,
// the solve kernel, which leaves the wrenches of the next launch, and forward dynamics again, whichever plan mh_aba_* takes.  Frames and
// scratch, rooted and _between_ alike: FrameList and con_scratch (mh_launch_plans.h); mh_reserve covers the rooted form at K = 8, the first
// call of a larger need grows the buffer (ensure_bytes), then the calls only enqueue.
static const double kNoGravity[3] = {0.0, 0.0, 0.0};
template <class ARGS>
void close_frames(const mh_model *m, FrameList &F, ARGS &G)
{ // closes the list and hands it to a solve kernel's arguments: the targets' poses, relative to their body-fixed frames, in the call's precision
   frame_list_close(*m, F);
   std::copy_n(F.tgt, F.K, G.tgt), std::copy_n(F.ext, F.K, G.ext), std::copy_n(F.base, F.K, G.base), std::copy_n(F.bext, F.K, G.bext);
   std::copy_n(F.bslot, F.K, G.bslot), std::copy_n(&F.pose[0][0], 12 * F.K, &G.pose[0][0]);
   G.K = F.K, G.n_app = F.n_app;
}
// per-body twists of (q, qd): the inverse dynamics' outward sweep (its efforts go to qd_out, which the last launches overwrite)
template <typename T>
mh_status body_twists(mh_model_t model, int64_t B, const T *q, const T *qd, const mh_options &of, T *out, T *body)
{
   return launch<T>(ALGO_RNEA, model, B, q, qd, qd, kNoGravity, nullptr, &of, out, body_outputs<T>(nullptr, body));
}
// the change of velocity: forward dynamics at rest, without gravity, under the impulses alone, into a cleared qd_out (it skips entries no
// joint owns); then qd_out += qd
template <typename T>
mh_status impulses_to_qd(mh_model_t model, int64_t B, const T *q, const T *qd, const T *wrench, T *zeros, const mh_options &of, T *out)
{
   hipStream_t stream = (hipStream_t)of.stream;
   const long n_out = (long)B * (long)model->nv;
   HIP_TRY(hipMemsetAsync(zeros, 0, (size_t)n_out * sizeof(T), stream));
   HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_out * sizeof(T), stream));
   const mh_status st = launch<T>(ALGO_ABA, model, B, q, zeros, zeros, kNoGravity, wrench, &of, out);
   if (st != MH_OK || n_out == 0)
      return st;
   hipLaunchKernelGGL((mh::add_in_place_kernel<T>), dim3((int)std::min<long>((n_out + 255) / 256, (long)model->cu_count * 8)), dim3(256), 0, stream, out,
                      qd, n_out);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// between: the _between_ entry points (base_joints may still be NULL = every base the root: the rooted launches, bit for bit)
template <typename T>
mh_status constrained_impl(bool velocity, mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext,
                           int32_t n_targets, const int32_t *target_joints, const double *target_poses, const int32_t *target_rows,
                           const int32_t *active, const T *des, const double &compliance, const mh_options *opts_in, T *out, T *lambda_out,
                           bool between = false, const int32_t *base_joints = nullptr)
{
   const char *call = between ? (velocity ? "mh_constraint_impulse_between" : "mh_aba_constrained_between")
                              : (velocity ? "mh_constraint_impulse" : "mh_aba_constrained");
   // the scratch below belongs to the CONTEXT of the call: resolve it before anything mutable is touched
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: %d joint(s) are acceleration sources: the constrained dynamics take none", call, model->n_locked);
   if (n_targets < 1 || n_targets > MH_MAX_CONSTRAINT_TARGETS)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: n_targets = %d is outside 1 ... %d", call, n_targets, MH_MAX_CONSTRAINT_TARGETS);
   if (!target_joints || !target_rows)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: target_joints / target_rows is NULL", call);
   if (!(compliance >= 0.0)) // (a NaN fails too)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: compliance must be >= 0", call);
   if (!velocity && !gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: gravity is NULL and no root acceleration is set", call);
   mh::ConRelArgs<T> G{}; // (the rooted launch takes its ConArgs part)
   const int K = n_targets;
   FrameList F{K, K};
   for (int k = 0; k < K; k++)
   {
      const int rk = target_rows[k];
      if ((st = frame_target(*model, F, k, target_joints[k], base_joints ? base_joints[k] : -1, target_poses, call, false)) != MH_OK)
         return st;
      if (rk < 0 || rk > 0x3f)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d: row mask 0x%x has bits beyond the six rows of a frame", call, k, (unsigned)rk);
      if ((st = target_frame<double>(model, F.tgt[k], F.pose[k], F.app_canon[k], call, k)) != MH_OK)
         return st;
      G.rows[k] = rk;
      for (int r = 0; r < 6; r++)
         if ((rk >> r) & 1)
            G.idx[G.rows_total++] = (signed char)(6 * k + r);
   }
   if (G.rows_total == 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: no row is constrained (every entry of target_rows is 0)", call);
   close_frames(model, F, G);
   const bool rel = F.n_app > K;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || (!velocity && !tau) || !out)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: NULL state / output pointer", call);
   const size_t n6 = (size_t)model->n * 6;
   {
      const size_t bv = (size_t)B * model->nv * sizeof(T), bd = (size_t)B * 6 * K * sizeof(T);
      const InRange ins[6] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, bv}, {"tau", tau, bv}, {"f_ext", f_ext, (size_t)B * n6 * sizeof(T)},
                              {"active", active, (size_t)B * K * sizeof(int32_t)}, {velocity ? "v_des" : "a_des", des, bd}};
      const OutRange outs[2] = {{velocity ? "qd_out" : "qdd_out", out, bv, 0u}, {velocity ? "impulse_out" : "lambda_out", lambda_out, bd, 0u}};
      if ((st = check_aliasing(call, ins, 6, outs, 2)) != MH_OK)
         return st;
   }
   const ConScratch S = con_scratch(model->n, model->nv, K, F.n_app, true);
   if ((st = ensure_bytes(model->con, (size_t)B * S.total * sizeof(T))) != MH_OK)
      return st;
   mh_options of = o; // the launches below see the state as it is: both switches of the inverse dynamics on
   of.consider_coriolis = 1, of.consider_accelerations = 1, of.use_root_acceleration = velocity ? 0 : o.use_root_acceleration;
   T *const con = (T *)model->con.ptr, *const W = con + B * S.W, *const body = con + B * S.body, *const wrench = con + B * S.wrench, *const twist = con + B * S.twist;
   st = velocity ? body_twists<T>(model, B, q, qd, of, out, body)
                 : launch<T>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, &of, out, body_outputs<T>(body, rel ? twist : nullptr));
   if (st != MH_OK || (st = apparent_inertia_launch<T>(model, B, q, F.n_app, F.app_joints, F.app_canon, true, o, W, true)) != MH_OK)
      return st;
   const bool soa = o.layout == MH_LAYOUT_SOA;
   G.m = dev_model<T>(model);
   G.B = B;
   G.q = q;
   set_strides(G.q_bs, G.q_es, soa, B, model->nq);
   G.body = body, G.fext = velocity ? nullptr : f_ext, G.wrench = wrench;
   set_strides(G.f_bs, G.f_es, soa, B, (long)n6);
   G.W = W, G.rhs = con + B * S.rhs, G.twist = twist, G.zpose = con + B * S.zpose; // (rooted: two empty blocks, which its launch does not take)
   G.active = active;
   set_strides(G.a_bs, G.a_es, soa, B, K);
   G.des = des, G.lambda = lambda_out;
   set_strides(G.d_bs, G.d_es, soa, B, 6L * K);
   G.eps = (T)compliance;
   if (!velocity)
      set_root_acceleration(G, o, gravity);
   G.velocity = velocity;
   const int grid = (int)std::max<long>(1, std::min<long>(groups_of(B), (long)model->cu_count * 8));
   if (rel)
      hipLaunchKernelGGL((mh::constraint_solve_kernel<T, true>), dim3(grid), dim3(64), 0, (hipStream_t)o.stream, G);
   else
      hipLaunchKernelGGL((mh::constraint_solve_kernel<T>), dim3(grid), dim3(64), 0, (hipStream_t)o.stream, static_cast<const mh::ConArgs<T> &>(G));
   HIP_TRY(hipGetLastError());
   if (!velocity)
      return launch<T>(ALGO_ABA, model, B, q, qd, tau, gravity, wrench, &of, out);
   return impulses_to_qd<T>(model, B, q, qd, wrench, con + B * S.zeros, of, out);
}
// Frictional contact impulses: the velocity form above with the contact solve between the launches; rhs holds b and the normals in the target frames
template <typename T>
mh_status contact_impl(mh_model_t model, int64_t B, const T *q, const T *qd, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                       const double *mu, const T *normals, const int32_t *active, const T *v_normal, const T *impulse_init, const double &compliance,
                       int32_t n_iterations, const mh_options *opts_in, T *out, T *impulse_out, T *residual_out, bool between = false,
                       const int32_t *base_joints = nullptr)
{
   const char *call = between ? "mh_contact_impulse_between" : "mh_contact_impulse";
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: %d joint(s) are acceleration sources: the contact dynamics take none", call, model->n_locked);
   if (n_targets < 1 || n_targets > MH_MAX_CONTACT_TARGETS)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: n_targets = %d is outside 1 ... %d", call, n_targets, MH_MAX_CONTACT_TARGETS);
   if (!target_joints || !mu)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: target_joints / mu is NULL", call);
   if (!(compliance >= 0.0)) // (a NaN fails too)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: compliance must be >= 0", call);
   if (n_iterations < 1 || n_iterations > MH_MAX_CONTACT_ITERATIONS)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: n_iterations = %d is outside 1 ... %d", call, n_iterations, MH_MAX_CONTACT_ITERATIONS);
   mh::ContactRelArgs<T> G{}; // (the rooted launch takes its ContactArgs part)
   const int K = n_targets;
   FrameList F{K, K};
   for (int k = 0; k < K; k++)
   {
      if ((st = frame_target(*model, F, k, target_joints[k], base_joints ? base_joints[k] : -1, target_poses, call, true)) != MH_OK)
         return st;
      uint64_t mu_bits; // (read as bits: the translation unit is compiled with -ffinite-math-only)
      std::memcpy(&mu_bits, &mu[k], sizeof mu_bits);
      if (mu_bits >= 0x7ff0000000000000ull && mu_bits != 0x8000000000000000ull) // infinite, NaN or negative
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d: the friction coefficient must be finite and >= 0", call, k);
      if (mu[k] > (double)std::numeric_limits<T>::max()) // (finite in fp64, not in T)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: target %d: the friction coefficient %g is beyond the range of the call's precision", call, k, mu[k]);
      if ((st = target_frame<double>(model, F.tgt[k], F.pose[k], F.app_canon[k], call, k)) != MH_OK)
         return st;
      G.mu[k] = (T)(mu[k] > 1.0 ? 1.0 / mu[k] : mu[k]); // contact_project works a cone wider than 45 degrees with 1 / mu: no finite mu overflows
      G.wide |= mu[k] > 1.0 ? 1u << k : 0u;
   }
   close_frames(model, F, G);
   const bool rel = F.n_app > K;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !out)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: NULL state / output pointer", call);
   const size_t n6 = (size_t)model->n * 6;
   {
      const size_t bv = (size_t)B * model->nv * sizeof(T), bk = (size_t)B * K * sizeof(T), bd = 6 * bk;
      const InRange ins[6] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, bv}, {"normals", normals, 3 * bk},
                              {"active", active, (size_t)B * K * sizeof(int32_t)}, {"v_normal", v_normal, bk}, {"impulse_init", impulse_init, bd}};
      const OutRange outs[3] = {{"qd_out", out, bv, 0u}, {"impulse_out", impulse_out, bd, 1u << 5}, {"residual_out", residual_out, (size_t)B * sizeof(T), 0u}};
      if ((st = check_aliasing(call, ins, 6, outs, 3)) != MH_OK)
         return st;
   }
   const ConScratch S = con_scratch(model->n, model->nv, K, F.n_app, false);
   if ((st = ensure_bytes(model->con, (size_t)B * S.total * sizeof(T))) != MH_OK)
      return st;
   const ContactPlan P = contact_plan(K, sizeof(T), model->contact_path, model->cu_count, B);
   static const void *const kernels[2][2][2] = { // [rel][kmax == 8][resident]
      {{(const void *)&mh::contact_solve_kernel<T, false, 4>, (const void *)&mh::contact_solve_kernel<T, true, 4>},
       {(const void *)&mh::contact_solve_kernel<T, false, 8>, (const void *)&mh::contact_solve_kernel<T, true, 8>}},
      {{(const void *)&mh::contact_solve_kernel<T, false, 4, true>, (const void *)&mh::contact_solve_kernel<T, true, 4, true>},
       {(const void *)&mh::contact_solve_kernel<T, false, 8, true>, (const void *)&mh::contact_solve_kernel<T, true, 8, true>}}};
   const void *kern = kernels[rel][P.kmax == 8][P.resident];
   if ((st = raise_lds_limit(model, kern, (size_t)P.lds)) != MH_OK)
      return st;
   mh_options of = o;
   of.consider_coriolis = 1, of.consider_accelerations = 1, of.use_root_acceleration = 0;
   T *const con = (T *)model->con.ptr, *const W = con + B * S.W, *const body = con + B * S.body, *const wrench = con + B * S.wrench;
   st = body_twists<T>(model, B, q, qd, of, out, body);
   if (st != MH_OK || (st = apparent_inertia_launch<T>(model, B, q, F.n_app, F.app_joints, F.app_canon, true, o, W, true)) != MH_OK)
      return st;
   const bool soa = o.layout == MH_LAYOUT_SOA;
   G.m = dev_model<T>(model);
   G.B = B;
   G.q = q;
   set_strides(G.q_bs, G.q_es, soa, B, model->nq);
   G.body = body, G.wrench = wrench;
   set_strides(G.f_bs, G.f_es, soa, B, (long)n6);
   G.W = W, G.Wrel = W, G.zpose = con + B * S.zpose, G.bvec = con + B * S.rhs, G.nvec = G.bvec + (size_t)B * 3 * K;
   G.active = active, G.v_normal = v_normal;
   set_strides(G.a_bs, G.a_es, soa, B, K);
   G.normals = normals;
   set_strides(G.n_bs, G.n_es, soa, B, 3L * K);
   G.init = impulse_init, G.impulse = impulse_out;
   set_strides(G.d_bs, G.d_es, soa, B, 6L * K);
   G.residual = residual_out;
   G.eps = (T)compliance;
   G.n_iter = n_iterations;
   void *args[] = {rel ? (void *)&G : (void *)static_cast<mh::ContactArgs<T> *>(&G)};
   HIP_TRY(hipLaunchKernel(kern, dim3(P.grid), dim3(64), args, (size_t)P.lds, (hipStream_t)o.stream));
   return impulses_to_qd<T>(model, B, q, qd, wrench, con + B * S.zeros, of, out);
}
// Inverse of the joint-space inertia matrix, all columns or a list of them: run-time-topology kernel, which writes every entry of its
// output -- no memset in front of it.  The listed columns travel as kernel arguments (resolved here to joint and place); the call
// uploads nothing and allocates nothing beyond the workspace mh_reserve covers.
static int minv_groups(int n_columns) { return (n_columns + mh::MINV_GROUP - 1) / mh::MINV_GROUP; }
// The launch: G.col filled where `listed`, opts resolved to its context (begin_call).  out_soa: Hinv_out is [nv n_columns][B] whatever
// the call's layout (the scratch of mh_joint_limit_impulse_*); the strides of q stay those of the layout.
template <typename T>
mh_status minv_launch(mh_model_t model, int64_t B, const T *q, mh::MinvArgs<T> &G, int n_columns, bool listed, const mh_options &opts, T *Hinv_out,
                      bool out_soa)
{
   const Launch L = plan_launch(model->cu_count, B);
   const int parts = launch_parts(model->cu_count, L, minv_groups(n_columns));
   const mh_status st = ensure_bytes(model->ws, lane_ws_bytes(model->resp_slots, L, parts, sizeof(T)));
   if (st != MH_OK)
      return st;
   mh::Args<T> &A = G.a;
   A = make_args<T>(model, B, opts);
   A.q = q, A.out = Hinv_out;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   set_strides(G.h_bs, G.h_es, out_soa || opts.layout == MH_LAYOUT_SOA, B, (long)model->nv * n_columns);
   G.info = model->d_resp_info, G.owner = model->d_minv_owner;
   G.zero_ofs = model->d_grav_zero_ofs, G.zero_cols = model->d_grav_zero_cols;
   G.slots = model->resp_slots, G.a_base = model->resp_a_base, G.u_base = model->resp_u_base;
   G.n_columns = n_columns, G.listed = listed;
   hipLaunchKernelGGL((mh::mass_matrix_inverse_kernel<T>), dim3(L.grid, parts), dim3(L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status mass_matrix_inverse_impl(mh_model_t model, int64_t B, const T *q, int32_t n_columns, const int32_t *columns, const mh_options *opts_in,
                                   T *Hinv_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   mh::MinvArgs<T> G{};
   if (columns)
   {
      if (n_columns < 1 || n_columns > MH_MAX_INVERSE_COLUMNS)
         return fail(MH_ERR_INVALID_ARGUMENT, "n_columns = %d is outside 1 ... %d", n_columns, MH_MAX_INVERSE_COLUMNS);
      for (int k = 0; k < n_columns; k++)
      {
         if (columns[k] < 0 || columns[k] >= model->nv)
            return fail(MH_ERR_INVALID_ARGUMENT, "column %d names DoF index %d (nv = %d)", k, columns[k], model->nv);
         G.col[k] = model->minv_owner[columns[k]];
      }
   }
   else
      n_columns = model->nv;
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !Hinv_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL configuration / output pointer");
   const long hsize = (long)model->nv * n_columns;
   {
      const InRange in{"q", q, (size_t)B * model->nq * sizeof(T)};
      const OutRange out{"Hinv_out", Hinv_out, (size_t)B * hsize * sizeof(T), 0u};
      if ((st = check_aliasing("mh_mass_matrix_inverse", &in, 1, &out, 1)) != MH_OK)
         return st;
   }
   return minv_launch<T>(model, B, q, G, n_columns, columns != nullptr, opts, Hinv_out, false);
}
// Joint-limit impulses: the listed columns of H^-1 at the DoFs of the limited joints into SoA scratch (the launch above), then the solve
// kernel (mh_limit_kernels.h), which also forms qd_out from those columns.  Two launches on the caller's stream; the first call of a
// batch grows the scratch (ensure_bytes), then the calls only enqueue.
template <typename T>
mh_status limit_impl(mh_model_t model, int64_t B, const T *q, const T *qd, int32_t n_limits, const int32_t *limit_joints, const double *lower,
                     const double *upper, const double &margin, const double &erp, const T *impulse_init, const double &compliance,
                     int32_t n_iterations, const mh_options *opts_in, T *out, T *impulse_out, T *residual_out)
{
   const char *call = "mh_joint_limit_impulse";
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: %d joint(s) are acceleration sources: the joint-limit solve takes none", call, model->n_locked);
   if (n_limits < 1 || n_limits > MH_MAX_LIMIT_JOINTS)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: n_limits = %d is outside 1 ... %d", call, n_limits, MH_MAX_LIMIT_JOINTS);
   if (!limit_joints || !lower || !upper)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: %s is NULL", call, !limit_joints ? "limit_joints" : (!lower ? "lower" : "upper"));
   auto finite_nonneg = [](const double &x) { return !nonfinite_bits(x) && x >= 0.0; }; // (bits: -ffinite-math-only)
   if (!finite_nonneg(margin))
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: margin must be finite and >= 0", call);
   if (!finite_nonneg(erp))
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: erp must be finite and >= 0", call);
   if (!finite_nonneg(compliance))
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: compliance must be finite and >= 0", call);
   if (n_iterations < 1 || n_iterations > MH_MAX_LIMIT_ITERATIONS)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: n_iterations = %d is outside 1 ... %d", call, n_iterations, MH_MAX_LIMIT_ITERATIONS);
   const int L = n_limits;
   mh::LimitArgs<T> G{};
   mh::MinvArgs<T> M{};
   for (int i = 0; i < L; i++)
   {
      const int joint = limit_joints[i];
      if (joint < 0 || joint >= model->n)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: limit_joints[%d] names joint %d (the model has %d joints)", call, i, joint, model->n);
      const int *mi = &model->meta[(size_t)model->engine_of[joint] * mh::MI_STRIDE];
      if (mi[mh::MI_TYPE] != mh::JT_REVOLUTE && mi[mh::MI_TYPE] != mh::JT_PRISMATIC)
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: limit_joints[%d]: joint %d is neither revolute nor prismatic", call, i, joint);
      for (int k = 0; k < i; k++)
         if (limit_joints[k] == joint)
            return fail(MH_ERR_INVALID_ARGUMENT, "%s: limit_joints[%d]: joint %d is listed twice", call, i, joint);
      if (nan_bits(lower[i]) || nan_bits(upper[i]))
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: lower / upper of limit %d is NaN", call, i);
      if (lower[i] > upper[i])
         return fail(MH_ERR_INVALID_ARGUMENT, "%s: limit %d: lower %g > upper %g", call, i, lower[i], upper[i]);
      G.dof[i] = model->dof_map[mi[mh::MI_DOF]], G.cfg[i] = model->cfg_map[mi[mh::MI_CFG]];
      G.lower[i] = (T)lower[i], G.upper[i] = (T)upper[i];
      M.col[i] = model->minv_owner[G.dof[i]];
   }
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !out)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s: %s is NULL", call, !q ? "q" : (!qd ? "qd" : "qd_out"));
   {
      const size_t bv = (size_t)B * model->nv * sizeof(T), bl = (size_t)B * L * sizeof(T);
      const InRange ins[3] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, bv}, {"impulse_init", impulse_init, bl}};
      const OutRange outs[3] = {{"qd_out", out, bv, 0u}, {"impulse_out", impulse_out, bl, 1u << 2}, {"residual_out", residual_out, (size_t)B * sizeof(T), 0u}};
      if ((st = check_aliasing(call, ins, 3, outs, 3)) != MH_OK)
         return st;
   }
   if ((st = ensure_bytes(model->con, (size_t)B * model->nv * L * sizeof(T))) != MH_OK)
      return st;
   const LimitPlan P = limit_plan(L, sizeof(T), model->limit_path, model->cu_count, B);
   const void *kern = P.resident ? (const void *)&mh::limit_solve_kernel<T, true> : (const void *)&mh::limit_solve_kernel<T, false>;
   if ((st = raise_lds_limit(model, kern, (size_t)P.lds)) != MH_OK)
      return st;
   T *const Hinv = (T *)model->con.ptr;
   if ((st = minv_launch<T>(model, B, q, M, L, true, o, Hinv, true)) != MH_OK)
      return st;
   const bool soa = o.layout == MH_LAYOUT_SOA;
   G.B = B, G.nv = model->nv, G.L = L, G.n_iter = n_iterations;
   G.q = q, G.qd = qd, G.out = out;
   set_strides(G.q_bs, G.q_es, soa, B, model->nq);
   set_strides(G.v_bs, G.v_es, soa, B, model->nv);
   G.Hinv = Hinv, G.init = impulse_init, G.impulse = impulse_out, G.residual = residual_out;
   set_strides(G.d_bs, G.d_es, soa, B, L);
   G.eps = (T)compliance, G.margin = (T)margin, G.erp = (T)erp;
   void *args[] = {(void *)&G};
   HIP_TRY(hipLaunchKernel(kern, dim3(P.grid), dim3(64), args, (size_t)P.lds, (hipStream_t)o.stream));
   return MH_OK;
}
// Inverse / forward dynamics with the inertial parameters of every configuration in the batch (mh_params_kernels.h): run-time-topology
// kernels in the model's own workspace plan.  AoS: pi is read in place (the kernel stages it through LDS); big batches of wide state
// matrices go through the transposed scratch copies of launch<T>, as the fixed-parameter run-time-topology calls do.
template <typename T>
mh_status parameters_impl(Algo algo, mh_model_t model, int64_t B, const T *q, const T *qd, const T *in3, const T *pi, const double *gravity,
                          const T *f_ext, const mh_options *opts_in, T *out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (algo == ALGO_ABA && model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: forward dynamics with inertial parameters takes none", model->n_locked);
   if (!pi)
      return fail(MH_ERR_INVALID_ARGUMENT, "pi is NULL");
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !in3 || !out || (!gravity && !opts.use_root_acceleration))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   {
      const size_t bq = (size_t)B * model->nq * sizeof(T), bv = (size_t)B * model->nv * sizeof(T), bj = (size_t)B * model->n * sizeof(T);
      const InRange ins[5] = {{"q", q, bq}, {"qd", qd, bv}, {algo == ALGO_RNEA ? "qdd" : "tau", in3, bv}, {"f_ext", f_ext, 6 * bj},
                              {"pi", pi, mh::PARAMS_PER_BODY * bj}};
      const OutRange o1 = {algo == ALGO_RNEA ? "tau_out" : "qdd_out", out, bv, model->q_may_be_out ? 7u : 6u};
      if ((st = check_aliasing(algo == ALGO_RNEA ? "mh_rnea_parameters" : "mh_aba_parameters", ins, 5, &o1, 1)) != MH_OK)
         return st;
   }
   st = ensure_workspace(model, B, sizeof(T));
   if (st != MH_OK)
      return st;
   const Launch L = plan_launch(model->cu_count, B);
   hipStream_t stream = (hipStream_t)opts.stream;
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   mh::ParamArgs<T> G{};
   mh::Args<T> &A = G.a;
   A = make_args<T>(model, B, opts, gravity);
   A.q = q, A.qd = qd, A.in3 = in3, A.fext = f_ext, A.out = out;
   A.ws = (T *)model->ws.ptr;
   A.ws_stride = L.lanes;
   G.pi = pi;
   set_strides(G.p_bs, G.p_es, soa, B, (long)model->n * mh::PARAMS_PER_BODY);
   T *t_out = nullptr;
   if (!soa && transposes(model, B))
   {
      const size_t nq = model->nq, nv = model->nv;
      st = ensure_bytes(model->tr, (size_t)B * (nq + 3 * nv) * sizeof(T));
      if (st != MH_OK)
         return st;
      T *t_q = (T *)model->tr.ptr, *t_qd = t_q + (size_t)B * nq, *t_in3 = t_qd + (size_t)B * nv;
      t_out = t_in3 + (size_t)B * nv;
      mh::transpose_rows<T>(q, t_q, (long)B, (long)nq, true, stream);
      mh::transpose_rows<T>(qd, t_qd, (long)B, (long)nv, true, stream);
      mh::transpose_rows<T>(in3, t_in3, (long)B, (long)nv, true, stream);
      A.q = t_q, A.qd = t_qd, A.in3 = t_in3, A.out = t_out;
      A.q_bs = 1, A.q_es = B, A.v_bs = 1, A.v_es = B;
   }
   if (algo == ALGO_RNEA)
      hipLaunchKernelGGL((mh::rnea_parameters_kernel<T>), dim3(L.grid), dim3(L.block), 0, stream, G);
   else
      hipLaunchKernelGGL((mh::aba_parameters_kernel<T>), dim3(L.grid), dim3(L.block), 0, stream, G);
   if (t_out)
      mh::transpose_rows<T>((const T *)t_out, out, (long)B, (long)model->nv, false, stream);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Derivatives of the inverse dynamics with respect to q and qd (mh_rnea_deriv_kernels.h): run-time-topology kernel, which writes every
// entry of its outputs -- no memset in front of it -- in a slot plan of its own (more per body than the model's common plan holds)
// the scratch mh_reserve sets aside for the forward form (Hinv and qdd the caller does not ask for) stays within this; a larger need is
// met at the first such call
constexpr size_t kDerivReserveCap = (size_t)4 << 30;
static size_t deriv_scratch_bytes(const mh_model *m, int64_t B, size_t elem) { return (size_t)B * ((size_t)m->nv * m->nv + (size_t)m->nv) * elem; }
static size_t step_scratch_bytes(const mh_model *m, int64_t B, size_t elem) { return (size_t)B * 2 * (size_t)m->nv * m->nv * elem; }
template <typename T>
mh_status rnea_derivatives_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const double *gravity, const T *f_ext,
                                const mh_options *opts_in, T *tau_out, T *dq_out, T *dqd_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (!gravity && !opts.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!dq_out && !dqd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "dtau_dq_out and dtau_dqd_out are both NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || (opts.consider_coriolis && !qd) || (opts.consider_accelerations && !qdd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer (qd may be NULL with consider_coriolis = 0, qdd with consider_accelerations = 0)");
   {
      const size_t nq = (size_t)B * model->nq * sizeof(T), nvb = (size_t)B * model->nv * sizeof(T), nm = nvb * model->nv,
                   nf = (size_t)B * model->n * 6 * sizeof(T);
      const InRange ins[4] = {{"q", q, nq}, {"qd", opts.consider_coriolis ? qd : nullptr, nvb}, {"qdd", opts.consider_accelerations ? qdd : nullptr, nvb},
                              {"f_ext", f_ext, nf}};
      const OutRange outs[3] = {{"tau_out", tau_out, nvb, 0u}, {"dtau_dq_out", dq_out, nm, 0u}, {"dtau_dqd_out", dqd_out, nm, 0u}};
      if ((st = check_aliasing("mh_rnea_derivatives", ins, 4, outs, 3)) != MH_OK)
         return st;
   }
   LaneSweep<T> S;
   if ((st = plan_lane_sweep<T>(model, B, opts, gravity, model->deriv_slots, S)) != MH_OK)
      return st;
   mh::DerivArgs<T> G{};
   mh::Args<T> &A = G.a = S.A;
   A.q = q, A.qd = qd, A.in3 = qdd, A.fext = f_ext, A.out = tau_out;
   G.dq = dq_out, G.dqd = dqd_out;
   set_strides(G.g_bs, G.g_es, opts.layout == MH_LAYOUT_SOA, B, (long)model->nv * model->nv);
   G.slot = model->d_deriv_slot, G.slots = model->deriv_slots;
   G.zero_ofs = model->d_grav_zero_ofs, G.zero_cols = model->d_grav_zero_cols;
   hipLaunchKernelGGL((mh::rnea_derivatives_kernel<T>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Derivatives of the forward dynamics: launches composed on the caller's stream -- forward dynamics (whichever plan mh_aba_* takes), the
// inverse-dynamics derivatives at that qdd straight into the caller's matrices, the full inverse mass matrix, and D <- -Hinv D in place.
template <typename T>
mh_status aba_derivatives_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext,
                                      const mh_options *opts_in, T *qdd_out, T *dq_out, T *dqd_out, T *Hinv_out)
{
   // the scratch below belongs to the CONTEXT of the call: resolve it before anything mutable is touched
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the derivatives of the forward dynamics take none", model->n_locked);
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!dq_out && !dqd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "dqdd_dq_out and dqdd_dqd_out are both NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !qd || !tau)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   if (model->nv > mh::NEG_SOLVE_LDS_ENTRIES) // one column of a matrix has to fit the product kernel's LDS buffer
      return fail(MH_ERR_INVALID_ARGUMENT, "nv = %d is beyond the %d DoFs the product kernel takes", model->nv, mh::NEG_SOLVE_LDS_ENTRIES);
   const size_t nvb = (size_t)B * model->nv * sizeof(T), nm = nvb * model->nv;
   {
      const InRange ins[4] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(T)}};
      const OutRange outs[4] = {{"qdd_out", qdd_out, nvb, 0u}, {"dqdd_dq_out", dq_out, nm, 0u}, {"dqdd_dqd_out", dqd_out, nm, 0u}, {"Hinv_out", Hinv_out, nm, 0u}};
      if ((st = check_aliasing("mh_aba_derivatives", ins, 4, outs, 4)) != MH_OK)
         return st;
   }
   T *qdd = qdd_out, *Hinv = Hinv_out;
   if (!qdd || !Hinv)
   {
      st = ensure_bytes(model->deriv, deriv_scratch_bytes(model, B, sizeof(T)));
      if (st != MH_OK)
         return st;
      if (!Hinv)
         Hinv = (T *)model->deriv.ptr;
      if (!qdd)
         qdd = (T *)model->deriv.ptr + (size_t)B * model->nv * model->nv;
   }
   st = launch<T>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, &o, qdd);
   if (st != MH_OK)
      return st;
   mh_options od = o; // the inverse dynamics at the state forward dynamics saw: both switches on
   od.consider_coriolis = 1, od.consider_accelerations = 1;
   st = rnea_derivatives_impl<T>(model, B, q, qd, qdd, gravity, f_ext, &od, nullptr, dq_out, dqd_out);
   if (st != MH_OK)
      return st;
   st = mass_matrix_inverse_impl<T>(model, B, q, 0, nullptr, &o, Hinv);
   if (st != MH_OK)
      return st;
   mh::NegSolveArgs<T> N{};
   N.Hinv = Hinv, N.D0 = dq_out ? dq_out : dqd_out, N.D1 = dq_out ? dqd_out : nullptr;
   N.B = B, N.nv = model->nv;
   set_strides(N.bs, N.es, o.layout == MH_LAYOUT_SOA, B, (long)model->nv * model->nv);
   N.kc = std::max(1, std::min(model->nv, mh::NEG_SOLVE_LDS_ENTRIES / model->nv));
   const int grid = (int)std::min<int64_t>(B, (int64_t)model->cu_count * 32);
   hipLaunchKernelGGL((mh::neg_hinv_product_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)o.stream, N);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Reverse-mode gradients of the inverse dynamics (mh_rnea_vjp_kernels.h): one launch of a run-time-topology kernel in a slot plan of its
// own, which writes every entry of the outputs it is given.  negate: -gq and -gqd (the forward form below).  accumulate: gq and gqd are
// added to what the outputs hold and entries no joint owns are left alone (mh_aba_integrate_vjp_*).
// The scratch of the forward forms: qdd and H^-1 w for mh_aba_vjp_*, which is given w; qdd, w and H^-1 w for mh_aba_integrate_vjp_*.
static size_t vjp_scratch_bytes(const mh_model *m, int64_t B, size_t elem, int vectors = 3) { return (size_t)B * vectors * (size_t)m->nv * elem; }
template <typename T>
mh_status rnea_vjp_launch(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const double *gravity, const T *f_ext, const T *u,
                          const mh_options &opts, bool negate, T *gq_out, T *gqd_out, T *gqdd_out, bool accumulate = false)
{
   LaneSweep<T> S;
   if (const mh_status st = plan_lane_sweep<T>(model, B, opts, gravity, model->vjp_slots, S); st != MH_OK)
      return st;
   mh::VjpArgs<T> G{};
   mh::Args<T> &A = G.a = S.A;
   A.q = q, A.qd = qd, A.in3 = qdd, A.fext = f_ext, A.out = nullptr;
   G.u = u, G.gq = gq_out, G.gqd = gqd_out, G.gqdd = gqdd_out;
   G.slot = model->d_vjp_slot, G.slots = model->vjp_slots;
   G.negate = negate, G.accumulate = accumulate;
   set_unowned(model, G.unowned, G.n_unowned);
   hipLaunchKernelGGL((mh::rnea_vjp_kernel<T>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status rnea_vjp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const double *gravity, const T *f_ext, const T *u,
                        const mh_options *opts_in, T *gq_out, T *gqd_out, T *gqdd_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the gradients of the dynamics take none", model->n_locked);
   if (!gravity && !opts.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!gq_out && !gqd_out && !gqdd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_out, gqd_out and gqdd_out are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !u || (opts.consider_coriolis && !qd) || (opts.consider_accelerations && !qdd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / cotangent pointer (qd may be NULL with consider_coriolis = 0, qdd with consider_accelerations = 0)");
   {
      const size_t nq = (size_t)B * model->nq * sizeof(T), nvb = (size_t)B * model->nv * sizeof(T), nf = (size_t)B * model->n * 6 * sizeof(T);
      const InRange ins[5] = {{"q", q, nq}, {"qd", opts.consider_coriolis ? qd : nullptr, nvb}, {"qdd", opts.consider_accelerations ? qdd : nullptr, nvb},
                              {"f_ext", f_ext, nf}, {"u", u, nvb}};
      const OutRange outs[3] = {{"gq_out", gq_out, nvb, 0u}, {"gqd_out", gqd_out, nvb, 0u}, {"gqdd_out", gqdd_out, nvb, 0u}};
      if ((st = check_aliasing("mh_rnea_vjp", ins, 5, outs, 3)) != MH_OK)
         return st;
   }
   return rnea_vjp_launch<T>(model, B, q, qd, qdd, gravity, f_ext, u, opts, false, gq_out, gqd_out, gqdd_out);
}
// ---- The forward form, shared by mh_aba_vjp_*, mh_aba_parameters_vjp_*, mh_aba_parameters_state_vjp_* and mh_aba_integrate_vjp_*: with
// tau = H qdd + b, the cotangent w of qdd gives gtau = mu = H^-1 w and the adjoint sweep of the inverse dynamics at (q, qd, qdd) with
// u = mu, negated, gives the rest.  Every such call resolves qdd and mu, runs forward_form and then its own adjoint launch.
//
// the options of the inverse dynamics at the state forward dynamics saw (and of the per-row forms' forward dynamics): both switches on
static mh_options both_switches_on(mh_options o)
{
   o.consider_coriolis = 1, o.consider_accelerations = 1;
   return o;
}
// qdd and mu: the caller's outputs, or two vectors of the context's vjp scratch -- qdd at 0 and mu at B nv, whichever is missing
template <typename T>
mh_status forward_form_scratch(mh_model *model, int64_t B, T *qdd_out, T *gtau_out, T *&qdd, T *&mu)
{
   qdd = qdd_out, mu = gtau_out;
   if (qdd && mu)
      return MH_OK;
   if (const mh_status st = ensure_bytes(model->vjp, vjp_scratch_bytes(model, B, sizeof(T), 2)); st != MH_OK)
      return st;
   if (!qdd)
      qdd = (T *)model->vjp.ptr;
   if (!mu)
      mu = (T *)model->vjp.ptr + (size_t)B * model->nv;
   return MH_OK;
}
// ... for the step, whose w is scratch as well: w first, then qdd and mu where the caller takes neither, 1 + !qdd_out + !gtau_out vectors
template <typename T>
mh_status step_form_scratch(mh_model *model, int64_t B, T *qdd_out, T *gtau_out, T *&w, T *&qdd, T *&mu)
{
   if (const mh_status st = ensure_bytes(model->vjp, vjp_scratch_bytes(model, B, sizeof(T), 1 + !qdd_out + !gtau_out)); st != MH_OK)
      return st;
   const size_t bn = (size_t)B * model->nv;
   w = (T *)model->vjp.ptr;
   qdd = qdd_out ? qdd_out : w + bn;
   mu = gtau_out ? gtau_out : (qdd_out ? w + bn : w + 2 * bn);
   return MH_OK;
}
// the forward dynamics of a call, as forward_form runs it: (qd, tau, gravity, f_ext, options, out) -> status, everything else bound.
// Fixed parameters: whichever plan mh_aba_* takes.  (The per-row forms bind parameters_impl and pi.)
template <typename T>
auto fixed_forward_dynamics(mh_model_t model, int64_t B, const T *q)
{
   return [=](const T *qd, const T *tau, const double *gravity, const T *f_ext, const mh_options &o, T *out) {
      return launch<T>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, &o, out);
   };
}
template <typename T>
auto per_row_forward_dynamics(mh_model_t model, int64_t B, const T *q, const T *pi)
{
   return [=](const T *qd, const T *tau, const double *gravity, const T *f_ext, const mh_options &o, T *out) {
      return parameters_impl<T>(ALGO_ABA, model, B, q, qd, tau, pi, gravity, f_ext, &o, out);
   };
}
static mh_status nothing_between() { return MH_OK; }
// The launches, composed on the caller's stream:
//   fd(qd, tau, gravity, f_ext) -> qdd with the options `first` -- the caller's, or both_switches_on (the per-row forms) -- unless
//                                  !run_first (only gtau is asked for, which needs no qdd);
//   between()                      the step's integrator launch, which forms w from that qdd; nothing elsewhere;
//   memset(mu), then fd IN PLACE at rest: qd = mu (zeroed first, so the scratch stays at two vectors), tau = w, out = mu, no gravity
//                                  pointer, a zero root acceleration in `first`'s options and no wrenches: mu = H^-1 w.
template <typename T, class FD, class Between>
mh_status forward_form(mh_model *model, int64_t B, const T *qd, const T *tau, const double *gravity, const T *f_ext, const T *w, const mh_options &first,
                       bool run_first, T *qdd, T *mu, FD fd, Between between)
{
   mh_status st;
   if (run_first)
      if ((st = fd(qd, tau, gravity, f_ext, first, qdd)) != MH_OK)
         return st;
   if ((st = between()) != MH_OK)
      return st;
   mh_options rest = first; // H^-1 w: nothing moves, nothing pulls
   rest.use_root_acceleration = 1;
   for (double &x : rest.root_acceleration)
      x = 0.0;
   HIP_TRY(hipMemsetAsync(mu, 0, (size_t)B * model->nv * sizeof(T), (hipStream_t)first.stream));
   return fd(mu, w, nullptr, nullptr, rest, mu);
}
// Reverse-mode gradients of the forward dynamics: three launches (and one memset) on the caller's stream -- forward_form with the
// fixed-parameter forward dynamics and the caller's options, then the kernel above at that qdd with u = mu, negated.  No matrix anywhere.
template <typename T>
mh_status aba_vjp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext, const T *w,
                       const mh_options *opts_in, T *qdd_out, T *gq_out, T *gqd_out, T *gtau_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the gradients of the dynamics take none", model->n_locked);
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!gq_out && !gqd_out && !gtau_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_out, gqd_out and gtau_out are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !qd || !tau || !w)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / cotangent pointer");
   const size_t nvb = (size_t)B * model->nv * sizeof(T);
   {
      const InRange ins[5] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(T)},
                              {"w", w, nvb}};
      const OutRange outs[4] = {{"qdd_out", qdd_out, nvb, 0u}, {"gq_out", gq_out, nvb, 0u}, {"gqd_out", gqd_out, nvb, 0u}, {"gtau_out", gtau_out, nvb, 0u}};
      if ((st = check_aliasing("mh_aba_vjp", ins, 5, outs, 4)) != MH_OK)
         return st;
   }
   T *qdd, *mu;
   if ((st = forward_form_scratch<T>(model, B, qdd_out, gtau_out, qdd, mu)) != MH_OK)
      return st;
   const bool need_qdd = qdd_out || gq_out || gqd_out; // (gtau_out alone needs no qdd)
   st = forward_form<T>(model, B, qd, tau, gravity, f_ext, w, o, need_qdd, qdd, mu, fixed_forward_dynamics<T>(model, B, q), nothing_between);
   if (st != MH_OK || (!gq_out && !gqd_out))
      return st;
   return rnea_vjp_launch<T>(model, B, q, qd, qdd, gravity, f_ext, mu, both_switches_on(o), true, gq_out, gqd_out, nullptr);
}
// Reverse-mode gradient of the inverse dynamics with respect to the per-configuration inertial parameters (mh_params_vjp_kernels.h): one
// launch of a run-time-topology kernel in the model's own workspace plan, up to min(8, n) waves per group of configurations on small
// batches (the first row of mh_reserve's lane plans), which writes every entry of gpi_out.  negate: -gpi (the forward form below).  Big AoS
// batches of wide state matrices go through the transposed scratch copies, as in parameters_impl; pi and gpi are staged by the kernel.
template <typename T>
mh_status parameters_vjp_launch(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const T *pi, const double *gravity, const T *u,
                                const mh_options &opts, bool negate, T *gpi_out)
{
   LaneSweep<T> S;
   mh_status st = plan_lane_sweep<T>(model, B, opts, gravity, model->n_slots, S);
   if (st != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   mh::ParamVjpArgs<T> G{};
   mh::Args<T> &A = G.p.a = S.A;
   A.q = q, A.qd = qd, A.in3 = qdd, A.fext = nullptr, A.out = nullptr;
   G.p.pi = pi, G.u = u, G.gpi = gpi_out, G.negate = negate;
   set_strides(G.p.p_bs, G.p.p_es, soa, B, (long)model->n * mh::PARAMS_PER_BODY);
   if (!soa && transposes(model, B))
   {
      const size_t nq = model->nq, nv = model->nv;
      st = ensure_bytes(model->tr, (size_t)B * (nq + 3 * nv) * sizeof(T));
      if (st != MH_OK)
         return st;
      T *t_q = (T *)model->tr.ptr, *t_qd = t_q + (size_t)B * nq, *t_qdd = t_qd + (size_t)B * nv, *t_u = t_qdd + (size_t)B * nv;
      mh::transpose_rows<T>(q, t_q, (long)B, (long)nq, true, stream);
      if (opts.consider_coriolis)
         mh::transpose_rows<T>(qd, t_qd, (long)B, (long)nv, true, stream);
      if (opts.consider_accelerations)
         mh::transpose_rows<T>(qdd, t_qdd, (long)B, (long)nv, true, stream);
      mh::transpose_rows<T>(u, t_u, (long)B, (long)nv, true, stream);
      A.q = t_q, A.qd = t_qd, A.in3 = t_qdd, G.u = t_u;
      A.q_bs = 1, A.q_es = B, A.v_bs = 1, A.v_es = B;
   }
   hipLaunchKernelGGL((mh::rnea_parameters_vjp_kernel<T>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status rnea_parameters_vjp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const T *pi, const double *gravity, const T *u,
                                   const mh_options *opts_in, T *gpi_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (!pi || !u || !gpi_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s is NULL", !pi ? "pi" : (!u ? "u" : "gpi_out"));
   if (B == 0)
      return MH_OK;
   if (!gravity && !opts.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!q || (opts.consider_coriolis && !qd) || (opts.consider_accelerations && !qdd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer (qd may be NULL with consider_coriolis = 0, qdd with consider_accelerations = 0)");
   {
      const size_t nq = (size_t)B * model->nq * sizeof(T), nvb = (size_t)B * model->nv * sizeof(T);
      const size_t np = (size_t)B * model->n * mh::PARAMS_PER_BODY * sizeof(T);
      const InRange ins[5] = {{"q", q, nq}, {"qd", opts.consider_coriolis ? qd : nullptr, nvb}, {"qdd", opts.consider_accelerations ? qdd : nullptr, nvb},
                              {"pi", pi, np}, {"u", u, nvb}};
      const OutRange out = {"gpi_out", gpi_out, np, 0u};
      if ((st = check_aliasing("mh_rnea_parameters_vjp", ins, 5, &out, 1)) != MH_OK)
         return st;
   }
   return parameters_vjp_launch<T>(model, B, q, qd, qdd, pi, gravity, u, opts, false, gpi_out);
}
// ... and of the forward dynamics: forward_form with the per-configuration forward dynamics (aba_parameters_kernel) and both switches
// on, which never skips its first launch here (gpi needs qdd), then the kernel above at that qdd with u = mu = H(pi)^-1 w, negated.
// External wrenches enter the first launch only: tau is affine in them.  The scratch: qdd and mu where the caller takes neither (two of
// the three vectors mh_reserve sets aside for the state gradients).  Unlike its neighbours the call goes on at nv = 0.
template <typename T>
mh_status aba_parameters_vjp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const T *pi, const double *gravity, const T *f_ext,
                                  const T *w, const mh_options *opts_in, T *qdd_out, T *gtau_out, T *gpi_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: forward dynamics with inertial parameters takes none", model->n_locked);
   if (!pi || !w || !gpi_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "%s is NULL", !pi ? "pi" : (!w ? "w" : "gpi_out"));
   if (B == 0)
      return MH_OK;
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!q || !qd || !tau)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   const size_t nvb = (size_t)B * model->nv * sizeof(T);
   {
      const size_t bj = (size_t)B * model->n * sizeof(T);
      const InRange ins[6] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"pi", pi, mh::PARAMS_PER_BODY * bj},
                              {"f_ext", f_ext, 6 * bj}, {"w", w, nvb}};
      const OutRange outs[3] = {{"qdd_out", qdd_out, nvb, 0u}, {"gtau_out", gtau_out, nvb, 0u}, {"gpi_out", gpi_out, mh::PARAMS_PER_BODY * bj, 0u}};
      if ((st = check_aliasing("mh_aba_parameters_vjp", ins, 6, outs, 3)) != MH_OK)
         return st;
   }
   const mh_options od = both_switches_on(o); // forward dynamics, and the inverse dynamics at the state it saw
   T *qdd = qdd_out, *mu = gtau_out;
   if (model->nv > 0) // (a model without DoFs has parameters all the same: no forward dynamics, and the kernel below writes its zeros)
   {
      if ((st = forward_form_scratch<T>(model, B, qdd_out, gtau_out, qdd, mu)) != MH_OK)
         return st;
      if ((st = forward_form<T>(model, B, qd, tau, gravity, f_ext, w, od, true, qdd, mu, per_row_forward_dynamics<T>(model, B, q, pi), nothing_between)) != MH_OK)
         return st;
   }
   return parameters_vjp_launch<T>(model, B, q, qd, qdd, pi, gravity, mu, od, true, gpi_out);
}
// State AND parameter gradients of the inverse dynamics at per-configuration parameters (mh_params_state_vjp_kernels.h): one launch of
// the adjoint sweep of rnea_vjp_launch with every body's inertia read from the row's pi, in that kernel's slot plan (vjp_slots: the fourth
// row of mh_reserve's lane plans) and with its parts; it writes every entry of the outputs it is given, the ten derivatives per body in
// its outward sweep when gpi_out is given.  The state matrices are read in place in both layouts, as rnea_vjp_launch reads them; pi and
// gpi are staged by the kernel.  negate: -gq, -gqd and -gpi (the forward form below).
template <typename T>
mh_status parameters_state_vjp_launch(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const T *pi, const double *gravity,
                                      const T *f_ext, const T *u, const mh_options &opts, bool negate, T *gq_out, T *gqd_out, T *gqdd_out, T *gpi_out)
{
   LaneSweep<T> S;
   if (const mh_status st = plan_lane_sweep<T>(model, B, opts, gravity, model->vjp_slots, S); st != MH_OK)
      return st;
   mh::ParamStateVjpArgs<T> G{};
   mh::Args<T> &A = G.pv.p.a = S.A;
   A.q = q, A.qd = qd, A.in3 = qdd, A.fext = f_ext, A.out = nullptr;
   G.pv.p.pi = pi, G.pv.u = u, G.pv.gpi = gpi_out, G.pv.negate = negate;
   set_strides(G.pv.p.p_bs, G.pv.p.p_es, opts.layout == MH_LAYOUT_SOA, B, (long)model->n * mh::PARAMS_PER_BODY);
   G.gq = gq_out, G.gqd = gqd_out, G.gqdd = gqdd_out;
   G.slot = model->d_vjp_slot, G.slots = model->vjp_slots;
   set_unowned(model, G.unowned, G.n_unowned);
   hipLaunchKernelGGL((mh::rnea_parameters_state_vjp_kernel<T>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status rnea_parameters_state_vjp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const T *pi, const double *gravity,
                                         const T *f_ext, const T *u, const mh_options *opts_in, T *gq_out, T *gqd_out, T *gqdd_out, T *gpi_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the gradients of the dynamics take none", model->n_locked);
   if (!pi)
      return fail(MH_ERR_INVALID_ARGUMENT, "pi is NULL");
   if (!gravity && !opts.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!gq_out && !gqd_out && !gqdd_out && !gpi_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_out, gqd_out, gqdd_out and gpi_out are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !u || (opts.consider_coriolis && !qd) || (opts.consider_accelerations && !qdd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / cotangent pointer (qd may be NULL with consider_coriolis = 0, qdd with consider_accelerations = 0)");
   {
      const size_t nq = (size_t)B * model->nq * sizeof(T), nvb = (size_t)B * model->nv * sizeof(T), bj = (size_t)B * model->n * sizeof(T);
      const InRange ins[6] = {{"q", q, nq}, {"qd", opts.consider_coriolis ? qd : nullptr, nvb}, {"qdd", opts.consider_accelerations ? qdd : nullptr, nvb},
                              {"pi", pi, mh::PARAMS_PER_BODY * bj}, {"f_ext", f_ext, 6 * bj}, {"u", u, nvb}};
      const OutRange outs[4] = {{"gq_out", gq_out, nvb, 0u}, {"gqd_out", gqd_out, nvb, 0u}, {"gqdd_out", gqdd_out, nvb, 0u},
                                {"gpi_out", gpi_out, mh::PARAMS_PER_BODY * bj, 0u}};
      if ((st = check_aliasing("mh_rnea_parameters_state_vjp", ins, 6, outs, 4)) != MH_OK)
         return st;
   }
   return parameters_state_vjp_launch<T>(model, B, q, qd, qdd, pi, gravity, f_ext, u, opts, false, gq_out, gqd_out, gqdd_out, gpi_out);
}
// ... and of the forward dynamics: forward_form with the per-configuration forward dynamics and both switches on, as in
// aba_parameters_vjp_impl, then the kernel above at that qdd with u = mu = H(pi)^-1 w = gtau, negated, which gives gq, gqd and gpi
// together.  The scratch: qdd and mu where the caller takes neither (two of the three vectors mh_reserve sets aside).
template <typename T>
mh_status aba_parameters_state_vjp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const T *pi, const double *gravity,
                                        const T *f_ext, const T *w, const mh_options *opts_in, T *qdd_out, T *gq_out, T *gqd_out, T *gtau_out,
                                        T *gpi_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the gradients of the dynamics take none", model->n_locked);
   if (!pi)
      return fail(MH_ERR_INVALID_ARGUMENT, "pi is NULL");
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!gq_out && !gqd_out && !gtau_out && !gpi_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_out, gqd_out, gtau_out and gpi_out are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !qd || !tau || !w)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / cotangent pointer");
   const size_t nvb = (size_t)B * model->nv * sizeof(T);
   {
      const size_t bj = (size_t)B * model->n * sizeof(T);
      const InRange ins[6] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"pi", pi, mh::PARAMS_PER_BODY * bj},
                              {"f_ext", f_ext, 6 * bj}, {"w", w, nvb}};
      const OutRange outs[5] = {{"qdd_out", qdd_out, nvb, 0u}, {"gq_out", gq_out, nvb, 0u}, {"gqd_out", gqd_out, nvb, 0u}, {"gtau_out", gtau_out, nvb, 0u},
                                {"gpi_out", gpi_out, mh::PARAMS_PER_BODY * bj, 0u}};
      if ((st = check_aliasing("mh_aba_parameters_state_vjp", ins, 6, outs, 5)) != MH_OK)
         return st;
   }
   T *qdd, *mu;
   if ((st = forward_form_scratch<T>(model, B, qdd_out, gtau_out, qdd, mu)) != MH_OK)
      return st;
   const mh_options od = both_switches_on(o); // forward dynamics, and the inverse dynamics at the state it saw
   const bool need_qdd = qdd_out || gq_out || gqd_out || gpi_out; // (gtau_out alone needs no qdd)
   st = forward_form<T>(model, B, qd, tau, gravity, f_ext, w, od, need_qdd, qdd, mu, per_row_forward_dynamics<T>(model, B, q, pi), nothing_between);
   if (st != MH_OK || (!gq_out && !gqd_out && !gpi_out))
      return st;
   return parameters_state_vjp_launch<T>(model, B, q, qd, qdd, pi, gravity, f_ext, mu, od, true, gq_out, gqd_out, nullptr, gpi_out);
}
template <typename T>
mh_status integrate_impl(mh_model_t model, int64_t B, double dt, const T *q, const T *qd, const T *qdd, const mh_options *opts_in, T *q_out,
                                T *qd_out, T *qdd_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !qdd || !q_out || !qd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   if (nan_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is NaN");
   { // the in-place step: every output may be its own input, nothing else
      const size_t bq = (size_t)B * model->nq * sizeof(T), bv = (size_t)B * model->nv * sizeof(T);
      const InRange ins[3] = {{"q", q, bq}, {"qd", qd, bv}, {"qdd", qdd, bv}};
      const OutRange outs[3] = {{"q_out", q_out, bq, 1u}, {"qd_out", qd_out, bv, 2u}, {"qdd_out", qdd_out, bv, 4u}};
      if ((st = check_aliasing("mh_integrate", ins, 3, outs, 3)) != MH_OK)
         return st;
   }
   mh::IntArgs<T> A;
   A.m = dev_model<T>(model);
   A.B = B, A.dt = (T)dt;
   A.q = q, A.qd = qd, A.qdd = qdd, A.q_out = q_out, A.qd_out = qd_out, A.qdd_out = qdd_out;
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   set_strides(A.q_bs, A.q_es, soa, B, model->nq);
   set_strides(A.v_bs, A.v_es, soa, B, model->nv);
   const int block = 256;
   if (soa)
   {
      const int grid = (int)std::max<long>(1, std::min<long>((B + block - 1) / block, (long)model->cu_count * 8));
      hipLaunchKernelGGL((mh::integrate_soa_kernel<T>), dim3(grid), dim3(block), 0, (hipStream_t)opts.stream, A);
   }
   else
   {
      // tile: enough workgroups to cover the device at small B, up to 256 configurations each at large B
      const int tile = (int)std::max<long>(16, std::min<long>(256, B / ((long)model->cu_count * 4)));
      const int grid = (int)std::max<long>(1, std::min<long>((B + tile - 1) / tile, (long)model->cu_count * 8));
      hipLaunchKernelGGL((mh::integrate_aos_kernel<T>), dim3(grid), dim3(block), ((size_t)model->n * 3 + 2) * sizeof(int), (hipStream_t)opts.stream, A, tile);
   }
   HIP_TRY(hipGetLastError());
   return MH_OK;
}

// q (+) dq and q1 (-) q0 (mh_step_kernels.h): one elementwise run-time-topology kernel each, no workspace
template <typename T>
mh::ChartArgs<T> chart_args(const mh_model *model, int64_t B, const mh_options &opts)
{
   mh::ChartArgs<T> A{};
   A.m = dev_model<T>(model);
   A.B = B;
   A.soa = opts.layout == MH_LAYOUT_SOA;
   set_strides(A.q_bs, A.q_es, A.soa, B, model->nq);
   set_strides(A.v_bs, A.v_es, A.soa, B, model->nv);
   set_unowned(model, A.unowned, A.n_unowned);
   return A;
}
static int chart_grid(const mh_model *model, int64_t B)
{
   return (int)std::max<int64_t>(1, std::min<int64_t>((B * std::max(model->n, model->nv) + 255) / 256, (int64_t)model->cu_count * 8));
}
template <typename T>
mh_status configuration_add_impl(mh_model_t model, int64_t B, const T *q, const T *dq, const mh_options *opts_in, T *q_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !dq || !q_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   {
      const InRange ins[2] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"dq", dq, (size_t)B * model->nv * sizeof(T)}};
      const OutRange out = {"q_out", q_out, (size_t)B * model->nq * sizeof(T), 1u};
      if ((st = check_aliasing("mh_configuration_add", ins, 2, &out, 1)) != MH_OK)
         return st;
   }
   mh::ChartArgs<T> A = chart_args<T>(model, B, opts);
   A.a = q, A.b = dq, A.out = q_out;
   hipLaunchKernelGGL((mh::configuration_add_kernel<T>), dim3(chart_grid(model, B)), dim3(256), 0, (hipStream_t)opts.stream, A);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status configuration_difference_impl(mh_model_t model, int64_t B, const T *q0, const T *q1, const mh_options *opts_in, T *dq_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q0 || !q1 || !dq_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   {
      const size_t bq = (size_t)B * model->nq * sizeof(T);
      const InRange ins[2] = {{"q0", q0, bq}, {"q1", q1, bq}};
      const OutRange out = {"dq_out", dq_out, (size_t)B * model->nv * sizeof(T), 0u};
      if ((st = check_aliasing("mh_configuration_difference", ins, 2, &out, 1)) != MH_OK)
         return st;
   }
   mh::ChartArgs<T> A = chart_args<T>(model, B, opts);
   A.a = q0, A.b = q1, A.out = dq_out;
   hipLaunchKernelGGL((mh::configuration_difference_kernel<T>), dim3(chart_grid(model, B)), dim3(256), 0, (hipStream_t)opts.stream, A);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
// Linearisation of the simulation step: launches composed on the caller's stream -- mh_aba_derivatives_* with both derivative matrices in
// the context's `step` scratch and H^-1 (and qdd, unless the caller takes it) in its `deriv` scratch, the assembly kernel of
// mh_step_kernels.h, and the integrator kernel when the new state is asked for.
template <typename T>
mh_status step_derivatives_impl(mh_model_t model, int64_t B, const double &dt, const T *q, const T *qd, const T *tau, const double *gravity,
                                const T *f_ext, const mh_options *opts_in, T *qdd_out, T *q_next, T *qd_next, T *A_out, T *B_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the linearisation of the step takes none", model->n_locked);
   if (nonfinite_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is not finite");
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (B == 0 || model->nv == 0) // (nothing to write: the pointers of empty matrices may well be NULL)
      return MH_OK;
   if (!A_out && !B_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "A_out and B_out are both NULL");
   if ((q_next == nullptr) != (qd_next == nullptr))
      return fail(MH_ERR_INVALID_ARGUMENT, "q_next and qd_next may be NULL only together");
   if (!q || !qd || !tau)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   if (model->nv > mh::NEG_SOLVE_LDS_ENTRIES)
      return fail(MH_ERR_INVALID_ARGUMENT, "nv = %d is beyond the %d DoFs mh_aba_derivatives takes", model->nv, mh::NEG_SOLVE_LDS_ENTRIES);
   const size_t nv = (size_t)model->nv, bv = (size_t)B * nv * sizeof(T), bq = (size_t)B * model->nq * sizeof(T);
   {
      const InRange ins[4] = {{"q", q, bq}, {"qd", qd, bv}, {"tau", tau, bv}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(T)}};
      const OutRange outs[5] = {{"qdd_out", qdd_out, bv, 0u}, {"q_next", q_next, bq, 0u}, {"qd_next", qd_next, bv, 0u},
                                {"A_out", A_out, 4 * bv * nv, 0u}, {"B_out", B_out, 2 * bv * nv, 0u}};
      if ((st = check_aliasing("mh_aba_integrate_derivatives", ins, 4, outs, 5)) != MH_OK)
         return st;
   }
   if ((st = ensure_bytes(model->step, step_scratch_bytes(model, B, sizeof(T)))) != MH_OK)
      return st;
   T *Dq = (T *)model->step.ptr, *Dv = Dq + (size_t)B * nv * nv;
   st = aba_derivatives_impl<T>(model, B, q, qd, tau, gravity, f_ext, &o, qdd_out, Dq, Dv, nullptr);
   if (st != MH_OK)
      return st;
   const bool soa = o.layout == MH_LAYOUT_SOA;
   hipStream_t stream = (hipStream_t)o.stream;
   mh::StepArgs<T> S{};
   S.m = dev_model<T>(model);
   S.B = B, S.dt = (T)dt;
   S.qd = qd, S.qdd = qdd_out ? qdd_out : (T *)model->deriv.ptr + (size_t)B * nv * nv;
   S.Dq = Dq, S.Dv = Dv, S.Hinv = (const T *)model->deriv.ptr;
   S.A = A_out, S.Bm = B_out;
   set_unowned(model, S.unowned, S.n_unowned);
   set_strides(S.v_bs, S.v_es, soa, B, (long)nv);
   set_strides(S.d_bs, S.d_es, soa, B, (long)(nv * nv));
   set_strides(S.a_bs, S.a_es, soa, B, (long)(4 * nv * nv));
   set_strides(S.b_bs, S.b_es, soa, B, (long)(2 * nv * nv));
   if (soa)
   {
      const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + 255) / 256, (int64_t)model->cu_count * 8));
      hipLaunchKernelGGL((mh::step_assemble_soa_kernel<T>), dim3(grid), dim3(256), 0, stream, S);
   }
   else
   {
      const int grid = (int)std::min<int64_t>(B, (int64_t)model->cu_count * 8);
      hipLaunchKernelGGL((mh::step_assemble_aos_kernel<T>), dim3(grid), dim3(256), 0, stream, S);
   }
   HIP_TRY(hipGetLastError());
   if (q_next)
      return integrate_impl<T>(model, B, dt, q, qd, S.qdd, &o, q_next, qd_next, nullptr);
   return MH_OK;
}
// Reverse mode of the integrator (mh_step_kernels.h: integrate_vjp_*_kernel): one elementwise launch in the integrator's own launch
// shape, no workspace.  Every entry of the outputs given is written once.
template <typename T>
mh_status integrate_vjp_launch(mh_model_t model, int64_t B, double dt, const T *qd, const T *qdd, const T *gq_next, const T *gqd_next,
                               const mh_options &opts, T *gq_out, T *gqd_out, T *gqdd_out)
{
   mh::StepVjpArgs<T> A{};
   A.m = dev_model<T>(model);
   A.B = B, A.dt = (T)dt;
   A.qd = qd, A.qdd = qdd, A.gqn = gq_next, A.gqdn = gqd_next;
   A.gq = gq_out, A.gqd = gqd_out, A.gqdd = gqdd_out;
   set_unowned(model, A.unowned, A.n_unowned);
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   set_strides(A.v_bs, A.v_es, soa, B, model->nv);
   const int block = 256;
   if (soa)
   {
      const int grid = (int)std::max<long>(1, std::min<long>((B + block - 1) / block, (long)model->cu_count * 8));
      hipLaunchKernelGGL((mh::integrate_vjp_soa_kernel<T>), dim3(grid), dim3(block), 0, (hipStream_t)opts.stream, A);
   }
   else
   { // the integrator's tiles: enough workgroups to cover the device at small B, up to 256 configurations each at large B
      const int tile = (int)std::max<long>(16, std::min<long>(256, B / ((long)model->cu_count * 4)));
      const int grid = (int)std::max<long>(1, std::min<long>((B + tile - 1) / tile, (long)model->cu_count * 8));
      hipLaunchKernelGGL((mh::integrate_vjp_aos_kernel<T>), dim3(grid), dim3(block), ((size_t)model->n * 2 + 2) * sizeof(int), (hipStream_t)opts.stream, A,
                         tile);
   }
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status integrate_vjp_impl(mh_model_t model, int64_t B, double dt, const T *qd, const T *qdd, const T *gq_next, const T *gqd_next,
                             const mh_options *opts_in, T *gq_out, T *gqd_out, T *gqdd_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (nonfinite_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is not finite");
   if (!gq_out && !gqd_out && !gqdd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_out, gqd_out and gqdd_out are all NULL");
   if (!gq_next && !gqd_next)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_next and gqd_next are both NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!qd || !qdd)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   {
      const size_t bv = (size_t)B * model->nv * sizeof(T);
      const InRange ins[4] = {{"qd", qd, bv}, {"qdd", qdd, bv}, {"gq_next", gq_next, bv}, {"gqd_next", gqd_next, bv}};
      const OutRange outs[3] = {{"gq_out", gq_out, bv, 0u}, {"gqd_out", gqd_out, bv, 0u}, {"gqdd_out", gqdd_out, bv, 0u}};
      if ((st = check_aliasing("mh_integrate_vjp", ins, 4, outs, 3)) != MH_OK)
         return st;
   }
   return integrate_vjp_launch<T>(model, B, dt, qd, qdd, gq_next, gqd_next, opts, gq_out, gqd_out, gqdd_out);
}
// Reverse mode of the step x' = integrate(q, qd, aba(q, qd, tau)): four launches (and one memset) composed on the caller's stream --
// forward_form as in aba_vjp_impl, with the kernel above between its two launches, which writes the integrator's own share of gq and
// gqd into the outputs and w = the cotangent of qdd into scratch; then the adjoint sweep at that qdd with u = mu = H^-1 w = gtau,
// negated, ADDING its gq and gqd to what the outputs hold (VjpArgs::accumulate).
template <typename T>
mh_status step_vjp_impl(mh_model_t model, int64_t B, double dt, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext,
                        const T *gq_next, const T *gqd_next, const mh_options *opts_in, T *qdd_out, T *gq_out, T *gqd_out, T *gtau_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the gradients of the step take none", model->n_locked);
   if (nonfinite_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is not finite");
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!gq_out && !gqd_out && !gtau_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_out, gqd_out and gtau_out are all NULL");
   if (!gq_next && !gqd_next)
      return fail(MH_ERR_INVALID_ARGUMENT, "gq_next and gqd_next are both NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !qd || !tau)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   const size_t nvb = (size_t)B * model->nv * sizeof(T);
   {
      const InRange ins[6] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(T)},
                              {"gq_next", gq_next, nvb}, {"gqd_next", gqd_next, nvb}};
      const OutRange outs[4] = {{"qdd_out", qdd_out, nvb, 0u}, {"gq_out", gq_out, nvb, 0u}, {"gqd_out", gqd_out, nvb, 0u}, {"gtau_out", gtau_out, nvb, 0u}};
      if ((st = check_aliasing("mh_aba_integrate_vjp", ins, 6, outs, 4)) != MH_OK)
         return st;
   }
   T *w, *qdd, *mu;
   if ((st = step_form_scratch<T>(model, B, qdd_out, gtau_out, w, qdd, mu)) != MH_OK)
      return st;
   // the first launch always runs (w needs qdd wherever dt != 0); the integrator's own launch sits between the two
   const auto integrator = [&] { return integrate_vjp_launch<T>(model, B, dt, qd, qdd, gq_next, gqd_next, o, gq_out, gqd_out, w); };
   st = forward_form<T>(model, B, qd, tau, gravity, f_ext, (const T *)w, o, true, qdd, mu, fixed_forward_dynamics<T>(model, B, q), integrator);
   if (st != MH_OK || (!gq_out && !gqd_out))
      return st;
   return rnea_vjp_launch<T>(model, B, q, qd, qdd, gravity, f_ext, mu, both_switches_on(o), true, gq_out, gqd_out, nullptr, true);
}
// ---- Forward mode (mh_rnea_jvp_kernels.h, mh_step_kernels.h: integrate_jvp_*_kernel): the matrices of the calls above times directions
// (dq, dqd, dqdd / dtau), none formed.
// The tangent sweep of the inverse dynamics: one launch in the kernel's own slot plan (fewer slots than rnea_vjp_launch's, which
// mh_reserve covers), which writes every entry of dtau_out once.  rhs: dtau_out = tau_in - dtau, a NULL tau_in being zero (the forward form
// below).
template <typename T>
mh_status rnea_jvp_launch(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const double *gravity, const T *f_ext, const T *dq,
                          const T *dqd, const T *dqdd, bool rhs, const T *tau_in, const mh_options &opts, T *dtau_out)
{
   LaneSweep<T> S;
   if (const mh_status st = plan_lane_sweep<T>(model, B, opts, gravity, model->jvp_slots, S); st != MH_OK)
      return st;
   mh::JvpArgs<T> G{};
   mh::Args<T> &A = G.a = S.A;
   A.q = q, A.qd = qd, A.in3 = qdd, A.fext = f_ext, A.out = dtau_out;
   G.dq = dq, G.dqd = dqd, G.dqdd = dqdd, G.rhs = rhs, G.tau_in = tau_in;
   G.slot = model->d_jvp_slot, G.slots = model->jvp_slots;
   set_unowned(model, G.unowned, G.n_unowned);
   hipLaunchKernelGGL((mh::rnea_jvp_kernel<T>), dim3(S.L.grid, S.parts), dim3(S.L.block), 0, (hipStream_t)opts.stream, G);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status rnea_jvp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *qdd, const double *gravity, const T *f_ext, const T *dq,
                        const T *dqd, const T *dqdd, const mh_options *opts_in, T *dtau_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the derivatives of the dynamics take none", model->n_locked);
   if (!gravity && !opts.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!dtau_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "dtau_out is NULL");
   if (!dq && !dqd && !dqdd)
      return fail(MH_ERR_INVALID_ARGUMENT, "dq, dqd and dqdd are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || (opts.consider_coriolis && !qd) || (opts.consider_accelerations && !qdd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer (qd may be NULL with consider_coriolis = 0, qdd with consider_accelerations = 0)");
   {
      const size_t nq = (size_t)B * model->nq * sizeof(T), nvb = (size_t)B * model->nv * sizeof(T), nf = (size_t)B * model->n * 6 * sizeof(T);
      const InRange ins[7] = {{"q", q, nq}, {"qd", opts.consider_coriolis ? qd : nullptr, nvb}, {"qdd", opts.consider_accelerations ? qdd : nullptr, nvb},
                              {"f_ext", f_ext, nf}, {"dq", dq, nvb}, {"dqd", opts.consider_coriolis ? dqd : nullptr, nvb}, {"dqdd", dqdd, nvb}};
      const OutRange out = {"dtau_out", dtau_out, nvb, 0u};
      if ((st = check_aliasing("mh_rnea_jvp", ins, 7, &out, 1)) != MH_OK)
         return st;
   }
   return rnea_jvp_launch<T>(model, B, q, qd, qdd, gravity, f_ext, dq, dqd, dqdd, false, nullptr, opts, dtau_out);
}
// Forward mode of the forward dynamics: with tau = H qdd + b, dqdd = H^-1 r, r = dtau - (d tau / d q) dq - (d tau / d qd) dqd at
// (q, qd, qdd).  forward_form with the tangent sweep as its `between`, which writes r into one vector of the context's vjp scratch:
// three launches (and one memset).  qdd: the caller's, or the vector before r.  Without dq and dqd r is dtau itself, the sweep is dropped
// and the first launch runs only for qdd_out.
template <typename T>
mh_status jvp_form_scratch(mh_model *model, int64_t B, bool sweep, T *qdd_out, T *&qdd, T *&r)
{
   qdd = qdd_out, r = nullptr;
   const int vectors = (sweep ? 1 : 0) + (sweep && !qdd_out ? 1 : 0);
   if (vectors == 0)
      return MH_OK;
   if (const mh_status st = ensure_bytes(model->vjp, vjp_scratch_bytes(model, B, sizeof(T), vectors)); st != MH_OK)
      return st;
   r = (T *)model->vjp.ptr;
   if (!qdd)
      qdd = r + (size_t)B * model->nv;
   return MH_OK;
}
template <typename T>
mh_status aba_jvp_run(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext, const T *dq,
                      const T *dqd, const T *dtau, const mh_options &o, T *qdd_out, T *qdd, T *r, T *dqdd_out)
{
   const bool sweep = dq || dqd;
   const auto tangent = [&] { return rnea_jvp_launch<T>(model, B, q, qd, qdd, gravity, f_ext, dq, dqd, (const T *)nullptr, true, dtau, both_switches_on(o), r); };
   if (sweep)
      return forward_form<T>(model, B, qd, tau, gravity, f_ext, (const T *)r, o, true, qdd, dqdd_out, fixed_forward_dynamics<T>(model, B, q), tangent);
   return forward_form<T>(model, B, qd, tau, gravity, f_ext, dtau, o, qdd_out != nullptr, qdd, dqdd_out, fixed_forward_dynamics<T>(model, B, q), nothing_between);
}
template <typename T>
mh_status aba_jvp_impl(mh_model_t model, int64_t B, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext, const T *dq,
                       const T *dqd, const T *dtau, const mh_options *opts_in, T *qdd_out, T *dqdd_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the derivatives of the dynamics take none", model->n_locked);
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!dqdd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "dqdd_out is NULL");
   if (!dq && !dqd && !dtau)
      return fail(MH_ERR_INVALID_ARGUMENT, "dq, dqd and dtau are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !qd || !tau)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   const size_t nvb = (size_t)B * model->nv * sizeof(T);
   {
      const InRange ins[7] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(T)},
                              {"dq", dq, nvb}, {"dqd", dqd, nvb}, {"dtau", dtau, nvb}};
      const OutRange outs[2] = {{"qdd_out", qdd_out, nvb, 0u}, {"dqdd_out", dqdd_out, nvb, 0u}};
      if ((st = check_aliasing("mh_aba_jvp", ins, 7, outs, 2)) != MH_OK)
         return st;
   }
   T *qdd, *r;
   if ((st = jvp_form_scratch<T>(model, B, dq || dqd, qdd_out, qdd, r)) != MH_OK)
      return st;
   return aba_jvp_run<T>(model, B, q, qd, tau, gravity, f_ext, dq, dqd, dtau, o, qdd_out, qdd, r, dqdd_out);
}
// Forward mode of the integrator: one elementwise launch in the integrator's own launch shape, no workspace.  Every entry of the
// outputs given is written once.
template <typename T>
mh_status integrate_jvp_launch(mh_model_t model, int64_t B, double dt, const T *qd, const T *qdd, const T *dq, const T *dqd, const T *dqdd,
                               const mh_options &opts, T *dq_next_out, T *dqd_next_out)
{
   mh::StepJvpArgs<T> A{};
   A.m = dev_model<T>(model);
   A.B = B, A.dt = (T)dt;
   A.qd = qd, A.qdd = qdd, A.dq = dq, A.dqd = dqd, A.dqdd = dqdd;
   A.dqn = dq_next_out, A.dqdn = dqd_next_out;
   set_unowned(model, A.unowned, A.n_unowned);
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   set_strides(A.v_bs, A.v_es, soa, B, model->nv);
   const int block = 256;
   if (soa)
   {
      const int grid = (int)std::max<long>(1, std::min<long>((B + block - 1) / block, (long)model->cu_count * 8));
      hipLaunchKernelGGL((mh::integrate_jvp_soa_kernel<T>), dim3(grid), dim3(block), 0, (hipStream_t)opts.stream, A);
   }
   else
   { // the integrator's tiles: enough workgroups to cover the device at small B, up to 256 configurations each at large B
      const int tile = (int)std::max<long>(16, std::min<long>(256, B / ((long)model->cu_count * 4)));
      const int grid = (int)std::max<long>(1, std::min<long>((B + tile - 1) / tile, (long)model->cu_count * 8));
      hipLaunchKernelGGL((mh::integrate_jvp_aos_kernel<T>), dim3(grid), dim3(block), ((size_t)model->n * 2 + 2) * sizeof(int), (hipStream_t)opts.stream, A,
                         tile);
   }
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
template <typename T>
mh_status integrate_jvp_impl(mh_model_t model, int64_t B, double dt, const T *qd, const T *qdd, const T *dq, const T *dqd, const T *dqdd,
                             const mh_options *opts_in, T *dq_next_out, T *dqd_next_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (nonfinite_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is not finite");
   if (!dq_next_out && !dqd_next_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "dq_next_out and dqd_next_out are both NULL");
   if (!dq && !dqd && !dqdd)
      return fail(MH_ERR_INVALID_ARGUMENT, "dq, dqd and dqdd are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!qd || !qdd)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   {
      const size_t bv = (size_t)B * model->nv * sizeof(T);
      const InRange ins[5] = {{"qd", qd, bv}, {"qdd", qdd, bv}, {"dq", dq, bv}, {"dqd", dqd, bv}, {"dqdd", dqdd, bv}};
      const OutRange outs[2] = {{"dq_next_out", dq_next_out, bv, 0u}, {"dqd_next_out", dqd_next_out, bv, 0u}};
      if ((st = check_aliasing("mh_integrate_jvp", ins, 5, outs, 2)) != MH_OK)
         return st;
   }
   return integrate_jvp_launch<T>(model, B, dt, qd, qdd, dq, dqd, dqdd, opts, dq_next_out, dqd_next_out);
}
// Forward mode of the step x' = integrate(q, qd, aba(q, qd, tau)): aba_jvp_run, then the integrator's tangent kernel on (dq, dqd, dqdd)
// at that qdd -- four launches (and one memset), exactly mh_aba_jvp_* followed by mh_integrate_jvp_*.  Scratch: r and qdd as in
// aba_jvp_impl, and dqdd behind them where the caller takes none -- at most three vectors of the context's vjp scratch.
template <typename T>
mh_status step_jvp_impl(mh_model_t model, int64_t B, double dt, const T *q, const T *qd, const T *tau, const double *gravity, const T *f_ext,
                        const T *dq, const T *dqd, const T *dtau, const mh_options *opts_in, T *qdd_out, T *dqdd_out, T *dq_next_out, T *dqd_next_out)
{
   mh_options o;
   mh_status st = begin_call(model, B, opts_in, o);
   if (st != MH_OK)
      return st;
   if (model->n_locked > 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "%d joint(s) are acceleration sources: the derivatives of the step take none", model->n_locked);
   if (nonfinite_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is not finite");
   if (!gravity && !o.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "gravity is NULL and no root acceleration is set");
   if (!dqdd_out && !dq_next_out && !dqd_next_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "dqdd_out, dq_next_out and dqd_next_out are all NULL");
   if (!dq && !dqd && !dtau)
      return fail(MH_ERR_INVALID_ARGUMENT, "dq, dqd and dtau are all NULL");
   if (B == 0 || model->nv == 0)
      return MH_OK;
   if (!q || !qd || !tau)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state pointer");
   const size_t nvb = (size_t)B * model->nv * sizeof(T);
   {
      const InRange ins[7] = {{"q", q, (size_t)B * model->nq * sizeof(T)}, {"qd", qd, nvb}, {"tau", tau, nvb}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(T)},
                              {"dq", dq, nvb}, {"dqd", dqd, nvb}, {"dtau", dtau, nvb}};
      const OutRange outs[4] = {{"qdd_out", qdd_out, nvb, 0u}, {"dqdd_out", dqdd_out, nvb, 0u}, {"dq_next_out", dq_next_out, nvb, 0u},
                                {"dqd_next_out", dqd_next_out, nvb, 0u}};
      if ((st = check_aliasing("mh_aba_integrate_jvp", ins, 7, outs, 4)) != MH_OK)
         return st;
   }
   // the integrator reads qdd wherever it runs, so the first launch always does: r, qdd and dqdd in this order, whichever is scratch
   const bool sweep = dq || dqd, integrator = dq_next_out || dqd_next_out;
   const int vectors = (sweep ? 1 : 0) + (qdd_out ? 0 : 1) + (dqdd_out ? 0 : 1);
   T *r = nullptr, *qdd = qdd_out, *dqdd = dqdd_out;
   if (vectors > 0)
   {
      if ((st = ensure_bytes(model->vjp, vjp_scratch_bytes(model, B, sizeof(T), vectors))) != MH_OK)
         return st;
      T *at = (T *)model->vjp.ptr;
      const size_t bn = (size_t)B * model->nv;
      if (sweep)
         r = at, at += bn;
      if (!qdd)
         qdd = at, at += bn;
      if (!dqdd)
         dqdd = at;
   }
   // (qdd_out as the "caller's wish" of aba_jvp_run: qdd is needed whenever the integrator runs)
   st = aba_jvp_run<T>(model, B, q, qd, tau, gravity, f_ext, dq, dqd, dtau, o, integrator ? qdd : qdd_out, qdd, r, dqdd);
   if (st != MH_OK || !integrator)
      return st;
   return integrate_jvp_launch<T>(model, B, dt, qd, (const T *)qdd, dq, dqd, (const T *)dqdd, o, dq_next_out, dqd_next_out);
}
} // namespace

static void self_check_spec(mh_model *m);
static mh_status build_code_object(const mh_model_desc *desc, const char *out_dir, char *path_out, size_t path_cap, bool fast);

// =================================================================================================== C-ABI
extern "C" {

int32_t mh_abi_version(void) { return MH_ABI_VERSION; }
uint64_t mh_spec_abi_stamp(void) { return mh::spec_abi_stamp(); }
const char *mh_build_hash(void) { return MH_STR_(MH_BUILD_HASH); }
const char *mh_spec_sources_hash(void) { return MH_STR_(MH_SPEC_SOURCES_HASH); }
mh_status mh_spec_sources_hash_of(const char *csrc_dir, char out[18])
{
   if (!csrc_dir || !out)
      return fail(MH_ERR_INVALID_ARGUMENT, "csrc_dir / out is NULL");
   if (!hash_spec_sources(csrc_dir, out))
      return fail(MH_ERR_INVALID_ARGUMENT, "%s does not hold the kernel sources (mh_spec.hip and its headers)", csrc_dir);
   return MH_OK;
}
const char *mh_last_error(void) { return g_err; }
// the library's other translation units (mh_comm.hip) report through the same thread-local message
mh_status mh_internal_fail(mh_status code, const char *message) { return fail(code, "%s", message); }
// What mh_model_create compiles from a description, for tests on machines without a device (not in include/mecano_hip.h either): runs
// plan_model and compile_model and copies out the member of ModelTables called `name` -- a vector under its own name (int32 or double
// entries), "scalars" (int32: n, nq, nv, n_slots, rnea_stack, aba_stack, pair_stack, aba_hand, n_nonadjacent, resp_slots, resp_a_base,
// resp_u_base, deriv_slots, ident_maps, dense_maps, q_may_be_out, warnings), "nonleaf_fraction" (one double), "topo_key" and "warning_text"
// (characters, no terminator).  *bytes_out is the table's size; `out` may be NULL to ask for it alone, otherwise capacity_bytes must hold it.
mh_status mh_internal_model_table(const mh_model_desc *desc, const char *name, void *out, size_t capacity_bytes, size_t *bytes_out)
{
   if (!name || !bytes_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "name / bytes_out is NULL");
   Plan P;
   ModelTables t;
   mh_status st = plan_model(desc, P);
   if (st == MH_OK)
      st = compile_model(desc, P, t);
   if (st != MH_OK)
      return st;
   const std::vector<int> scalars = {t.n, t.nq, t.nv, t.n_slots, t.rnea_stack, t.aba_stack, t.pair_stack, t.aba_hand, t.n_nonadjacent, t.resp_slots, t.resp_a_base,
                                     t.resp_u_base, t.deriv_slots, t.ident_maps, t.dense_maps, t.q_may_be_out, (int)t.warnings};
   struct Named
   {
      const char *name;
      const void *data;
      size_t bytes;
   };
   auto ints = [](const char *nm, const std::vector<int> &v) { return Named{nm, v.data(), v.size() * sizeof(int)}; };
   auto doubles = [](const char *nm, const std::vector<double> &v) { return Named{nm, v.data(), v.size() * sizeof(double)}; };
   auto chars = [](const char *nm, const std::string &v) { return Named{nm, v.data(), v.size()}; };
   const Named tables[] = {ints("scalars", scalars), ints("meta", t.meta), ints("dof_map", t.dof_map), ints("cfg_map", t.cfg_map), ints("engine_of", t.engine_of),
                           ints("prog", t.prog), ints("prog_seq", t.prog_seq), ints("grav_zero_ofs", t.grav_zero_ofs), ints("grav_zero_cols", t.grav_zero_cols),
                           ints("resp_info", t.resp_info), ints("minv_owner", t.minv_owner), ints("deriv_slot", t.deriv_slot), doubles("consts", t.consts),
                           doubles("sub_mass", t.sub_mass), doubles("inertial_parameters", t.inertial_parameters),
                           Named{"nonleaf_fraction", &t.nonleaf_fraction, sizeof(double)}, chars("topo_key", t.topo_key), chars("warning_text", t.warning_text)};
   for (const Named &row : tables)
      if (strcmp(row.name, name) == 0)
      {
         *bytes_out = row.bytes;
         if (out && capacity_bytes < row.bytes)
            return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_model_table: %s takes %zu bytes, the buffer holds %zu", name, row.bytes, capacity_bytes);
         if (out)
            std::memcpy(out, row.data, row.bytes);
         return MH_OK;
      }
   return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_model_table: no table called %s", name);
}
// What the planners of mh_launch_plans.h make of a description's tables, for the same tests (tests/test_launch_plans_cpu.py): runs
// plan_model, compile_model and the planner called `plan` on `params`, and copies out its result as int32 words, with the protocol above.
//   "dfs_frames"       (algo 0 | 1 | 2, budget, greedy): lds_slots, glb_slots, glb_frames, then the adapted body records
//   "dfs_choice"       (cu_count, algo 0 | 1, elem 4 | 8, B, aos, pair, dfs_place, dfs_budget): win; per_cu, budget, hand, b_win, slot_bytes,
//                      hand_lds, occ3 (dfs_choose); lds_slots, glb_slots, glb_frames of that budget's frames; lds, per_cu, grid, gslots, mode
//                      (dfs_geometry)
//   "split_rt"         (): usable, n_trunk, n_limbs, slots, est, total, n_seg[4], the sizes of trunk_list, seg, xl_ofs, xl and patches, then
//                      those five
//   "split_rt_records" (k 0 | 1 | 2): lds_slots, the sizes of meta and xl, then those two (a model with a usable split only)
//   "split_rt_shape"   (cu_count, elem, algo 0 | 1 | 2, B, pair): k, mode, lds, grid (a model with a usable split only)
//   "lane_ws"          (cu_count, B, want): block, grid, lanes of plan_launch; launch_parts; lane_ws_bytes and lane_ws_bound of one slot of
//                      one byte (the bound with B and want as the largest batch and want)
//   "constraint_frames" (K, K target joints, K base joints with -1 = the root body, twists wanted 0 | 1): the status of a refused list, or n_app,
//                      tgt[K], base[K], bslot[K], app_joints[n_app] (FrameList), then the offsets W, rhs, body, wrench, zeros, zpose, twist, total (con_scratch)
mh_status mh_internal_launch_plan(const mh_model_desc *desc, const char *plan, const int64_t *params, int32_t n_params, void *out, size_t capacity_bytes,
                                  size_t *bytes_out)
{
   if (!plan || !bytes_out || (n_params > 0 && !params))
      return fail(MH_ERR_INVALID_ARGUMENT, "plan / bytes_out / params is NULL");
   Plan P;
   ModelTables t;
   mh_status st = plan_model(desc, P);
   if (st == MH_OK)
      st = compile_model(desc, P, t);
   if (st != MH_OK)
      return st;
   const std::string name = plan;
   auto takes = [&](int count) { return n_params == count; };
   auto among = [&](int i, std::initializer_list<int64_t> allowed) { return std::find(allowed.begin(), allowed.end(), params[i]) != allowed.end(); };
   const char *const bad = "mh_internal_launch_plan: %s does not take these parameters";
   std::vector<int> w;
   auto append = [&](const std::vector<int> &v) { w.insert(w.end(), v.begin(), v.end()); };
   if (name == "dfs_frames")
   {
      if (!takes(3) || !among(0, {0, 1, 2}) || params[1] < 0 || params[1] > (1 << 16) || !among(2, {0, 1}))
         return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
      const FramePlan f = dfs_frames(t.meta, t.n, (int)params[0], (int)params[1], params[2] != 0);
      w = {f.lds_slots, f.glb_slots, f.glb_frames};
      append(f.meta);
   }
   else if (name == "dfs_choice")
   {
      if (!takes(8) || params[0] < 1 || params[0] > (1 << 20) || !among(1, {0, 1}) || !among(2, {4, 8}) || params[3] < 0 || !among(4, {0, 1}) || !among(5, {0, 1})
          || (params[5] && (params[1] != 1 || params[2] != 4)) || !among(6, {-1, 0, 1, 2}) || params[7] < -1 || params[7] > (1 << 16))
         return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
      Switches sw;
      sw.cu_count = (int)params[0], sw.dfs_place = (int)params[6], sw.dfs_budget = (int)params[7];
      const Algo algo = params[1] == 0 ? ALGO_RNEA : ALGO_ABA;
      const size_t elem = (size_t)params[2];
      const bool pair = params[5] != 0, win = !pair && dfs_windows(t, algo, elem, params[4] != 0);
      const DfsChoice c = dfs_choose(t, sw, algo, elem, params[3], win, pair);
      const FramePlan f = dfs_frames(t.meta, t.n, pair ? 2 : (algo == ALGO_RNEA ? 0 : 1), (int)c.budget, sw.dfs_place_greedy);
      const DfsGeometry g = dfs_geometry(c, f.lds_slots, f.glb_slots, f.glb_frames, groups_of(params[3]), sw.cu_count);
      w = {win, (int)c.per_cu, (int)c.budget, (int)c.hand, (int)c.b_win, (int)c.slot_bytes, c.hand_lds, c.occ3, f.lds_slots, f.glb_slots, f.glb_frames,
           (int)g.lds, (int)g.per_cu, g.grid, (int)g.gslots, g.mode};
   }
   else if (name == "split_rt" || name == "split_rt_records" || name == "split_rt_shape")
   {
      const SplitPlan S = split_rt_plan(t.meta, t.n, t.n_slots);
      if (name == "split_rt")
      {
         if (!takes(0))
            return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
         w = {S.usable, S.n_trunk, S.n_limbs, S.slots, S.est, S.total};
         w.insert(w.end(), S.n_seg, S.n_seg + mh::SPLIT_WAVES);
         for (const std::vector<int> *v : {&S.trunk_list, &S.seg, &S.xl_ofs, &S.xl, &S.patches})
            w.push_back((int)v->size());
         for (const std::vector<int> *v : {&S.trunk_list, &S.seg, &S.xl_ofs, &S.xl, &S.patches})
            append(*v);
      }
      else if (!S.usable)
         return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_launch_plan: %s: the tree has no usable run-time split", plan);
      else if (name == "split_rt_records")
      {
         if (!takes(1) || !among(0, {0, 1, 2}))
            return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
         const SplitRecords R = split_rt_records(S, t.meta, t.n, (int)params[0]);
         w = {R.lds_slots, (int)R.meta.size(), (int)R.xl.size()};
         append(R.meta), append(R.xl);
      }
      else
      {
         if (!takes(5) || params[0] < 1 || params[0] > (1 << 20) || !among(1, {4, 8}) || !among(2, {0, 1, 2}) || params[3] < 0 || !among(4, {0, 1}))
            return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
         int lds_slots[3];
         for (int k = 0; k < 3; k++)
            lds_slots[k] = split_rt_records(S, t.meta, t.n, k).lds_slots;
         const SplitShape s = split_rt_shape(S.slots, lds_slots, (int)params[0], (size_t)params[1], (Algo)params[2], params[3], params[4] != 0);
         w = {s.k, s.mode, (int)s.lds, s.grid};
      }
   }
   else if (name == "contact_solve")
   { // (K, bytes per element, force, CUs, batch)
      if (!takes(5) || params[0] < 1 || params[0] > MH_MAX_CONTACT_TARGETS || !among(1, {4, 8}) || !among(2, {-1, 0, 1}) || params[3] < 1
          || params[3] > (1 << 20) || params[4] < 0)
         return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
      const ContactPlan c = contact_plan((int)params[0], (size_t)params[1], (int)params[2], (int)params[3], params[4]);
      w = {c.resident, (int)c.lds, c.per_cu, c.grid, c.kmax};
   }
   else if (name == "limit_solve")
   { // (L, bytes per element, force, CUs, batch)
      if (!takes(5) || params[0] < 1 || params[0] > MH_MAX_LIMIT_JOINTS || !among(1, {4, 8}) || !among(2, {-1, 0, 1}) || params[3] < 1
          || params[3] > (1 << 20) || params[4] < 0)
         return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
      const LimitPlan c = limit_plan((int)params[0], (size_t)params[1], (int)params[2], (int)params[3], params[4]);
      w = {c.resident, (int)c.lds, c.per_cu, c.grid};
   }
   else if (name == "constraint_frames")
   {
      if (n_params < 1 || params[0] < 1 || params[0] > MH_MAX_CONSTRAINT_TARGETS || !takes(2 * (int)params[0] + 2) || !among(n_params - 1, {0, 1}))
         return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
      const int K = (int)params[0];
      auto joint = [&](int i) { return (int)std::clamp<int64_t>(params[i], -2, INT32_MAX); }; // (what no int holds is no joint of any model)
      FrameList F{K, K};
      for (int k = 0; k < K; k++)
         if ((st = frame_target(t, F, k, joint(1 + k), joint(1 + K + k), nullptr, plan, false)) != MH_OK)
            return st;
      frame_list_close(t, F);
      const ConScratch s = con_scratch(t.n, t.nv, K, F.n_app, params[2 * K + 1] != 0);
      w = {F.n_app};
      w.insert(w.end(), F.tgt, F.tgt + K), w.insert(w.end(), F.base, F.base + K), w.insert(w.end(), F.bslot, F.bslot + K);
      w.insert(w.end(), F.app_joints, F.app_joints + F.n_app);
      for (size_t entry : {s.W, s.rhs, s.body, s.wrench, s.zeros, s.zpose, s.twist, s.total})
         w.push_back((int)entry);
   }
   else if (name == "lane_ws")
   {
      if (!takes(3) || params[0] < 1 || params[0] > (1 << 20) || params[1] < 0 || params[1] > (1 << 30) || params[2] < 1 || params[2] > 4096)
         return fail(MH_ERR_INVALID_ARGUMENT, bad, plan);
      const int cus = (int)params[0];
      const Launch L = plan_launch(cus, params[1]);
      const int parts = launch_parts(cus, L, (long)params[2]);
      w = {L.block, L.grid, (int)L.lanes, parts, (int)lane_ws_bytes(1, L, parts, 1), (int)lane_ws_bound(cus, 1, L, (long)params[2], 1)};
   }
   else
      return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_launch_plan: no plan called %s", plan);
   *bytes_out = w.size() * sizeof(int);
   if (out && capacity_bytes < *bytes_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_launch_plan: %s takes %zu bytes, the buffer holds %zu", plan, *bytes_out, capacity_bytes);
   if (out)
      std::memcpy(out, w.data(), *bytes_out);
   return MH_OK;
}

mh_status mh_device_count(int32_t *count)
{
   if (!count)
      return fail(MH_ERR_INVALID_ARGUMENT, "count is NULL");
   int c = 0;
   if (hipGetDeviceCount(&c) != hipSuccess)
      c = 0;
   *count = c;
   return MH_OK;
}
mh_status mh_set_device(int32_t device)
{
   HIP_TRY(hipSetDevice(device));
   return MH_OK;
}
void mh_options_default(mh_options *opts)
{
   if (!opts)
      return;
   opts->consider_coriolis = 1;
   opts->consider_accelerations = 1;
   opts->layout = MH_LAYOUT_AOS;
   opts->use_root_acceleration = 0;
   opts->stream = nullptr;
   for (int k = 0; k < 6; k++)
      opts->root_acceleration[k] = 0.0;
   opts->context = nullptr;
}

mh_status mh_model_create(const mh_model_desc *d, mh_model_t *model_out)
{
   if (!d || !model_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "desc / model_out is NULL");
   *model_out = nullptr;
   Plan P;
   mh_status st = plan_model(d, P);
   if (st != MH_OK)
      return st;
   mh_model *m = new mh_model();
   st = compile_model(d, P, *m);
   if (st != MH_OK)
   {
      delete m;
      return st;
   }
   int dev = 0, ndev = 0;
   const hipError_t dc = hipGetDeviceCount(&ndev);
   if (dc != hipSuccess || ndev == 0)
   {
      delete m;
      return fail(MH_ERR_NO_DEVICE, "no HIP device (%s, %d device(s)): the model cannot be uploaded (there is no CPU path)", hipGetErrorString(dc), ndev);
   }
   hipError_t e = hipGetDevice(&dev);
   if (e == hipSuccess)
   {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, dev) == hipSuccess)
         m->cu_count = prop.multiProcessorCount;
   }
   m->device = dev;
   m->vjp_slots = vjp_slot_plan(m->meta, m->n, m->vjp_slot);
   m->jvp_slots = jvp_slot_plan(m->meta, m->n, m->jvp_slot);
   const std::vector<float> c32(m->consts.begin(), m->consts.end()), sm32(m->sub_mass.begin(), m->sub_mass.end());
   for (const DeviceRow &r : device_rows(m, c32, sm32))
   {
      if (e == hipSuccess)
         e = hipMalloc(r.ptr, r.bytes);
      if (e == hipSuccess)
         e = hipMemcpy(*r.ptr, r.host, r.bytes, hipMemcpyHostToDevice);
   }
   if (e != hipSuccess)
   {
      mh_model_destroy(m);
      return fail(MH_ERR_HIP, "model upload failed: %s", hipGetErrorString(e));
   }
   // fp64 forward dynamics at device-filling batches: the sweep kernel accumulates the children of a branching body through the workspace
   // (read-modify-write per extra child), the depth-first one keeps them on its stack -- measured on the reference's 30-joint shapes at
   // B = 262 144 (profiles/r02_generic_fp64_rates.txt): random trees 1253 -> 989 us and 1384 -> 1288 us on the depth-first kernel, chains
   // and the humanoid (4 branches in 24 joints) 3-12 % faster on the sweep.  Bushy = at least three branching bodies in ten.
   m->dfs_aba64 = m->n_nonadjacent * 10 >= 3 * std::max(1, m->n - 1);
   read_switches(*m); // after the device's CU count and the heuristic above: MH_FAKE_CU_COUNT and MH_DFS_ABA64 override them
   if (m->use_split_rt != 0)
      split_rt_create(m);
   try_load_spec(m, P);
   // MH_AUTO_BUILD: no usable code object for this tree (none there, or one refused for its ABI stamp / tree) -> build one now (hipcc on the
   // box; 1: the fast form, seconds; 2: the full set, minutes -- also when only a minimal object was found)
   if (const char *ab = getenv("MH_AUTO_BUILD"); ab && atoi(ab) != 0 && m->use_spec
                                                 && ((!m->spec.handle && m->variant.compare(0, 7, "generic") == 0) || (atoi(ab) == 2 && m->spec.handle && m->spec_minimal)))
   {
      char built[1024];
      if (m->spec.handle)
      { // a minimal object is loaded and the full set was asked for
         dlclose(m->spec.handle);
         m->spec = SpecLib{};
      }
      if (build_code_object(d, getenv("MH_SPEC_DIR"), built, sizeof built, atoi(ab) != 2) == MH_OK)
         try_load_spec(m, P);
      else
         m->variant = std::string("generic (MH_AUTO_BUILD: ") + g_err + ")";
   }
   if (!m->use_spec)
      m->variant = "generic";
   if (m->split_rt.usable && m->variant.compare(0, 7, "generic") == 0)
   {
      char buf[160];
      snprintf(buf, sizeof buf, "; small batches: run-time tree split over 4 waves (%d trunk bodies + %d limbs, path %d of %d body steps)", m->split_rt.n_trunk,
               m->split_rt.n_limbs, m->split_rt.est, m->split_rt.total);
      m->variant += buf;
   }
   int selfcheck = 1;
   if (const char *e = getenv("MH_SPEC_SELFCHECK"))
      selfcheck = atoi(e);
   if (m->spec.handle && m->use_spec && selfcheck)
      self_check_spec(m);
   if (m->warnings)
      (void)fail(MH_OK, "warning: %s", m->warning_text.c_str()); // (text for mh_last_error; the status stays MH_OK)
   *model_out = m;
   return MH_OK;
}

// the device records, the code object and the host-side description: released once, by whoever holds the last reference
static void release_model(mh_model *m)
{
   dfs_plans_drop(m);
   split_rt_free(m);
   for (const DeviceRow &r : device_rows(m))
      (void)hipFree(*r.ptr);
   free_scratch(*m);
   if (m->spec.handle)
      dlclose(m->spec.handle);
   delete m;
}
// The model is reference-counted by its contexts: they share its device records, so a model destroyed while contexts are alive only
// gives up the caller's reference (its handle must not be used again); the last mh_context_destroy releases everything.
void mh_model_destroy(mh_model_t m)
{
   if (!m)
      return;
   if (m->parent)
      return; // (the inner handle of a context cannot reach a caller; should one ever be passed here, its model owns the device records)
   {
      std::lock_guard<std::mutex> lock(g_context_mutex);
      if (m->destroy_pending)
         return; // destroyed twice
      if (m->n_contexts > 0)
      {
         m->destroy_pending = true;
         return;
      }
   }
   release_model(m);
}
// ---- contexts: the model handle is read-only and may be shared by any number of host threads and streams, each calling through a
//      context of its own ("Threading"; the reference keeps this state inside the calculator object, which is why
//      it needs one calculator per thread: InverseDynamicsCalculator.java:706-707)
mh_status mh_context_create(mh_model_t model, mh_context_t *ctx_out)
{
   if (!model || !ctx_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "model / ctx_out is NULL");
   *ctx_out = nullptr;
   mh_model *root = model->parent ? model->parent : model;
   mh_model *c = nullptr;
   {
      std::lock_guard<std::mutex> lock(g_context_mutex);
      if (root->destroy_pending)
         return fail(MH_ERR_INVALID_ARGUMENT, "mh_context_create: the model has been destroyed (it lives on only for its remaining contexts)");
      // The copy reads the immutable description only: what the default context's calls (or another context's first depth-first call, under
      // dfs_mutex) may be inserting into at this moment -- dfs_plans, lds_attr, pairs_host -- is FreshOnCopy and starts empty here; the
      // plain scratch words (Workspace, streams, events) are overwritten by the fresh ContextState below whatever was read.
      c = new (std::nothrow) mh_model(*root);
      if (!c)
         return fail(MH_ERR_OUT_OF_MEMORY, "out of host memory");
      root->n_contexts++;
   }
   c->parent = root;
   c->n_contexts = 0;
   c->destroy_pending = false;
   static_cast<ContextState &>(*c) = ContextState{}; // (its FreshOnCopy members came out of the copy empty: assignment leaves those alone)
   mh_context *ctx = new (std::nothrow) mh_context{c};
   if (!ctx)
   {
      delete c;
      std::lock_guard<std::mutex> lock(g_context_mutex);
      root->n_contexts--;
      return fail(MH_ERR_OUT_OF_MEMORY, "out of host memory");
   }
   *ctx_out = ctx;
   return MH_OK;
}
void mh_context_destroy(mh_context_t ctx)
{
   if (!ctx)
      return;
   mh_model *c = ctx->m;
   mh_model *root = c->parent;
   free_scratch(*c);
   bool last = false;
   {
      std::lock_guard<std::mutex> lock(g_context_mutex);
      last = --root->n_contexts == 0 && root->destroy_pending;
   }
   delete c;
   delete ctx;
   if (last)
      release_model(root); // mh_model_destroy came first: this was the last reference
}
mh_status mh_context_reserve(mh_context_t ctx, int64_t max_batch)
{
   if (!ctx)
      return fail(MH_ERR_INVALID_ARGUMENT, "context is NULL");
   return mh_reserve(ctx->m, max_batch);
}
// Synchronises `stream` and reports what the asynchronous calls issued through this context (NULL: the model's own) left behind.
mh_status mh_model_check(mh_model_t model, mh_context_t ctx, void *stream)
{
   if (!model)
      return fail(MH_ERR_INVALID_ARGUMENT, "model is NULL");
   mh_model *m = ctx ? ctx->m : model;
   if (ctx && m->parent != (model->parent ? model->parent : model))
      return fail(MH_ERR_INVALID_ARGUMENT, "the context belongs to another model");
   HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
   return zv_check_error(m);
}
mh_status mh_topology_key(const mh_model_desc *desc, char key_out[17], int32_t *parents_out, int32_t *types_out)
{
   Plan P;
   mh_status st = plan_model(desc, P);
   if (st != MH_OK)
      return st;
   if (key_out)
      snprintf(key_out, 17, "%s", P.key.c_str());
   for (int e = 0; e < desc->n_joints; e++)
   {
      if (parents_out)
         parents_out[e] = P.eparent[e];
      if (types_out)
         types_out[e] = P.etype[e];
   }
   return MH_OK;
}
int32_t mh_model_nq(mh_model_t m) { return m ? m->nq : -1; }
int32_t mh_model_nv(mh_model_t m) { return m ? m->nv : -1; }
int32_t mh_model_n_joints(mh_model_t m) { return m ? m->n : -1; }
mh_status mh_model_inertial_parameters(mh_model_t model, double *pi_out)
{
   if (!model)
      return fail(MH_ERR_INVALID_ARGUMENT, "model is NULL");
   if (!pi_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "pi_out is NULL");
   std::copy(model->inertial_parameters.begin(), model->inertial_parameters.end(), pi_out);
   return MH_OK;
}
const char *mh_model_kernel_variant(mh_model_t m) { return m ? m->variant.c_str() : ""; }
uint32_t mh_model_warnings(mh_model_t m) { return m ? m->warnings : 0u; }
const char *mh_model_warning_text(mh_model_t m) { return m ? m->warning_text.c_str() : ""; }

// Builds the topology-specialised code object of a model with hipcc (what mecano_amd/build.py does), for hosts without Python.
mh_status mh_build_code_object(const mh_model_desc *desc, const char *out_dir, char *path_out, size_t path_cap)
{
   return build_code_object(desc, out_dir, path_out, path_cap, getenv("MH_BUILD_FAST") && atoi(getenv("MH_BUILD_FAST")) != 0);
}
static mh_status build_code_object(const mh_model_desc *desc, const char *out_dir, char *path_out, size_t path_cap, bool fast)
{
   Plan P;
   mh_status st = plan_model(desc, P);
   if (st != MH_OK)
      return st;
   const int n = desc->n_joints;
   std::vector<int> depth(n, 0);
   int deepest = 0;
   for (int e = 0; e < n; e++)
   {
      if (P.etype[e] > MH_JOINT_FIXED)
         return fail(MH_ERR_UNSUPPORTED_JOINT, "specialised code objects cover revolute, prismatic, 6-DoF and fixed joints; planar / spherical joints run on the run-time-topology kernels");
      depth[e] = 1 + (P.eparent[e] >= 0 ? depth[P.eparent[e]] : 0);
      deepest = std::max(deepest, depth[e]);
   }
   if (deepest > 16)
      return fail(MH_ERR_BAD_TOPOLOGY, "the tree is %d joints deep: a compile-time walk stops paying beyond 16 (512 registers plus hundreds of spills); such models run on the run-time-topology kernels", deepest);
   Dl_info info;
   if (!dladdr((const void *)&mh_build_code_object, &info) || !info.dli_fname)
      return fail(MH_ERR_INVALID_ARGUMENT, "cannot locate libmecano_hip.so");
   std::string dir(info.dli_fname);
   const size_t slash = dir.find_last_of('/');
   dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
   const std::string src = dir + "/csrc/mh_spec.hip";
   if (FILE *f = fopen(src.c_str(), "r"))
      fclose(f);
   else
      return fail(MH_ERR_INVALID_ARGUMENT, "%s not found: the kernel sources must sit next to the library (csrc/)", src.c_str());
   char src_hash[18];
   if (!hash_spec_sources(dir + "/csrc", src_hash))
      return fail(MH_ERR_INVALID_ARGUMENT, "%s/csrc does not hold all the kernel sources", dir.c_str());
   if (strcmp(src_hash, MH_STR_(MH_SPEC_SOURCES_HASH)) != 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "the kernel sources in %s/csrc (hash %s) are not the ones this library was built beside (%s): the code object would be refused at load; rebuild the library",
                  dir.c_str(), src_hash, MH_STR_(MH_SPEC_SOURCES_HASH));
   // The compiler is clang++ itself, not the hipcc wrapper: hipcc assembles a command line of its own and hands it to a shell, so a
   // directory name with shell syntax in it would be interpreted there (seen in tests/test_abi.py).  MH_HIPCC overrides the choice.
   const char *hipcc = getenv("MH_HIPCC");
   std::string cc = hipcc ? hipcc : "";
   if (cc.empty())
   {
      for (const char *candidate : {"/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"})
         if (FILE *f = fopen(candidate, "r"))
         {
            fclose(f);
            cc = candidate;
            break;
         }
      if (cc.empty())
         cc = "amdclang++";
   }
   const size_t base = cc.find_last_of('/');
   const bool wrapper = cc.compare(base == std::string::npos ? 0 : base + 1, std::string::npos, "hipcc") == 0; // a user's MH_HIPCC=hipcc: its own driver flags
   std::string parents, kinds;
   for (int e = 0; e < n; e++)
   {
      parents += (e ? "," : "") + std::to_string(P.eparent[e]);
      kinds += (e ? "," : "") + std::to_string(P.etype[e]);
   }
   // A fast build (-DMH_SPEC_MINIMAL: tree-split RNEA / ABA / pair kernels for AoS matrices with identity index maps only) gets a name of
   // its own, so that it can neither be taken for the full object by mecano_amd.build (which would never build the full set then) nor
   // replace a full object; the loader prefers the full object and falls back to the minimal one.
   const std::string out = std::string(out_dir ? out_dir : dir.c_str()) + "/libmecano_hip_topo_" + P.key + (fast ? ".min.so" : ".so");
   const std::string tmp = out + ".tmp" + std::to_string((long)getpid());
   // hipcc is started WITHOUT a shell (posix_spawn with an argument vector): a directory name or flag handed in by an application cannot
   // be interpreted as shell syntax.  MH_HIPCC_FLAGS is split at white space into separate arguments.
   // (the flags of mecano_amd/build.py's SPEC_FLAGS: see there for -disable-machine-licm)
   std::vector<std::string> argv_s = {cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fno-signed-zeros", "-ffinite-math-only",
                                      "-fno-slp-vectorize", "-mllvm", "-disable-machine-licm"};
   if (!wrapper)
   {
      argv_s.push_back("--driver-mode=g++");
      argv_s.push_back("--hip-link");
   }
   if (fast)
      argv_s.push_back("-DMH_SPEC_MINIMAL");
   argv_s.push_back(std::string("-DMH_SPEC_SOURCES_HASH=") + src_hash);
   {
      // what else shaped this object (the fast form, a caller's extra flags): part of the build id its file carries
      uint64_t xh = fnv1a(0xcbf29ce484222325ull, fast ? "-DMH_SPEC_MINIMAL" : "", fast ? 17 : 0);
      if (const char *extra = getenv("MH_HIPCC_FLAGS"))
         xh = fnv1a(xh, extra, strlen(extra));
      char xs[48];
      snprintf(xs, sizeof xs, "-DMH_BUILD_EXTRA=h%016llx", (unsigned long long)xh);
      argv_s.push_back(xs);
   }
   if (const char *extra = getenv("MH_HIPCC_FLAGS"))
   {
      std::string word;
      for (const char *c = extra;; c++)
      {
         if (*c == 0 || *c == ' ' || *c == '\t' || *c == '\n')
         {
            if (!word.empty())
               argv_s.push_back(word);
            word.clear();
            if (*c == 0)
               break;
         }
         else
            word += *c;
      }
   }
   argv_s.push_back("-DMH_TOPO_N=" + std::to_string(n));
   argv_s.push_back("-DMH_TOPO_PARENTS=" + parents);
   argv_s.push_back("-DMH_TOPO_TYPES=" + kinds);
   argv_s.push_back("-o");
   argv_s.push_back(tmp);
   if (!wrapper)
   {
      argv_s.push_back("-x");
      argv_s.push_back("hip");
   }
   argv_s.push_back(src);
   std::vector<char *> argv;
   for (std::string &a : argv_s)
      argv.push_back(const_cast<char *>(a.c_str()));
   argv.push_back(nullptr);
   pid_t pid = 0;
   const int sp = posix_spawnp(&pid, cc.c_str(), nullptr, nullptr, argv.data(), environ);
   if (sp != 0)
      return fail(MH_ERR_HIP, "cannot start %s: %s", cc.c_str(), strerror(sp));
   int status = 0;
   while (waitpid(pid, &status, 0) < 0)
      if (errno != EINTR)
         return fail(MH_ERR_HIP, "waiting for %s failed: %s", cc.c_str(), strerror(errno));
   if (!WIFEXITED(status) || WEXITSTATUS(status) != 0)
   {
      (void)unlink(tmp.c_str());
      if (WIFEXITED(status))
         return fail(MH_ERR_HIP, "building the code object failed: %s exited with status %d", cc.c_str(), WEXITSTATUS(status));
      return fail(MH_ERR_HIP, "building the code object failed: %s was ended by signal %d", cc.c_str(), WIFSIGNALED(status) ? WTERMSIG(status) : -1);
   }
   if (rename(tmp.c_str(), out.c_str()) != 0) // atomic: a concurrent build of the same tree cannot leave a torn file
   {
      (void)unlink(tmp.c_str());
      return fail(MH_ERR_HIP, "cannot move the code object to %s: %s", out.c_str(), strerror(errno));
   }
   if (path_out && path_cap)
      snprintf(path_out, path_cap, "%s", out.c_str());
   return MH_OK;
}

mh_status mh_reserve(mh_model_t m, int64_t max_batch)
{
   mh_status st = check_common(m, max_batch, nullptr);
   if (st != MH_OK)
      return st;
   st = ensure_workspace(m, max_batch, sizeof(double)); // (mh_rnea_parameters_* / mh_aba_parameters_* work in this plan too)
   if (st != MH_OK)
      return st;
   { // the lane-workspace kernels: (slots per lane, the most waves per group of configurations a call may want), bounded over every
      // batch up to max_batch (lane_ws_bound; swept by tests/test_launch_plans_cpu.py)
      const Launch L = plan_launch(m->cu_count, max_batch);
      const long lane_plans[5][2] = {
         // mh_regressor_*, mh_crba_coriolis_*, mh_centroidal_*, mh_gravity_gradient_*, the mass matrix, mh_rnea_parameters_vjp_* /
         // mh_aba_parameters_vjp_* (the model's own slots: a branching body parks nu where the inverse dynamics parks its force)
         {m->n_slots, std::min(8, m->n)},
         // mh_apparent_inertia_inverse_*: its own slots behind the model's, up to one wave per target; mh_mass_matrix_inverse_* works in
         // the same slots with up to one wave per group of six columns
         {m->resp_slots, std::max<long>(MH_MAX_APPARENT_TARGETS, minv_groups(std::max<int>(m->nv, MH_MAX_INVERSE_COLUMNS)))},
         {m->deriv_slots, std::min(8, m->n)}, // mh_rnea_derivatives_* / mh_aba_derivatives_*: the kernel's own slot plan
         // mh_rnea_vjp_* / mh_aba_vjp_*: likewise; mh_rnea_parameters_state_vjp_* / mh_aba_parameters_state_vjp_* work in the same plan
         // (mh_rnea_jvp_* / mh_aba_jvp_*: a plan of fewer slots for every body, JS_BODY < VS_BODY and JS_BRANCH < VS_BRANCH, at the same waves)
         {m->vjp_slots, std::min(8, m->n)},
         // mh_body_poses_* / mh_geometric_jacobian_*: pose and twist of every body per lane, up to one wave per target
         {(long)m->n * mh::KIN_SLOTS, MH_MAX_KINEMATIC_TARGETS}};
      for (const auto &plan : lane_plans)
         if ((st = ensure_bytes(m->ws, lane_ws_bound(m->cu_count, plan[0], L, plan[1], sizeof(double)))) != MH_OK)
            return st;
      // mh_aba_derivatives_*: the scratch of the forward form
      if (m->nv > 0 && deriv_scratch_bytes(m, max_batch, sizeof(double)) <= kDerivReserveCap)
         st = ensure_bytes(m->deriv, deriv_scratch_bytes(m, max_batch, sizeof(double)));
      // mh_aba_vjp_* / mh_aba_integrate_vjp_*: qdd, w and H^-1 w, should the caller take neither qdd nor gtau (mh_aba_parameters_vjp_* /
      // mh_aba_parameters_state_vjp_*: the first two of the three)
      if (st == MH_OK && m->nv > 0)
         st = ensure_bytes(m->vjp, vjp_scratch_bytes(m, max_batch, sizeof(double)));
      // mh_aba_integrate_derivatives_*: the two derivative matrices beside them, under the same cap
      if (st == MH_OK && m->nv > 0 && deriv_scratch_bytes(m, max_batch, sizeof(double)) + step_scratch_bytes(m, max_batch, sizeof(double)) <= kDerivReserveCap)
         st = ensure_bytes(m->step, step_scratch_bytes(m, max_batch, sizeof(double)));
      if (st != MH_OK)
         return st;
      // mh_body_poses_* / mh_geometric_jacobian_*: the SoA form of their AoS outputs for the largest target list, while it stays within
      // the cap of the scratch above
      // (mh_body_poses_vjp_* / mh_jacobian_transpose_*: the cotangents of that many poses and nv entries behind them -- more than the
      // above only for a model with many fixed joints)
      const size_t kin_entries = std::max({kin_scratch_entries(m, MH_MAX_KINEMATIC_TARGETS, true, true), kin_scratch_entries(m, std::max(m->n, MH_MAX_KINEMATIC_TARGETS), false, false),
                                           kin_vjp_scratch_entries(m, std::max(m->n, MH_MAX_KINEMATIC_TARGETS), false)});
      if ((size_t)max_batch * kin_entries * sizeof(double) <= kDerivReserveCap)
         st = ensure_bytes(m->kin, (size_t)max_batch * kin_entries * sizeof(double));
      if (st != MH_OK)
         return st;
      // mh_aba_constrained_* / mh_constraint_impulse_*: their scratch for the largest target list, under the same cap
      const size_t con_bytes = (size_t)max_batch * con_scratch(m->n, m->nv, MH_MAX_CONSTRAINT_TARGETS, MH_MAX_CONSTRAINT_TARGETS, false).total * sizeof(double);
      if (con_bytes <= kDerivReserveCap && (st = ensure_bytes(m->con, con_bytes)) != MH_OK)
         return st;
   }
   // the whole-tree specialised ABA keeps its hand-over store in the same workspace (more slots than the run-time-topology plan of a
   // chain), and big AoS batches of wide matrices go through transposed scratch copies: reserve both, so that compute calls allocate nothing
   if (m->spec.aba_slots)
   {
      const Launch L = plan_launch(m->cu_count, max_batch);
      st = ensure_bytes(m->ws, (size_t)std::max(m->n_slots, m->spec.aba_slots()) * (size_t)L.lanes * sizeof(double));
      if (st != MH_OK)
         return st;
   }
   const bool transposed = transposes(m, max_batch);
   if (transposed)
      st = ensure_bytes(m->tr, (size_t)max_batch * ((size_t)m->nq + 3 * (size_t)m->nv) * sizeof(double));
   if (st != MH_OK)
      return st;
   // the depth-first kernels: every frame plan a batch of up to max_batch configurations can get, with the global blocks behind it and
   // its kernel's LDS attribute (dfs_setup).  A plan is cached per LDS budget, and dfs_choose picks the budget from the waves per CU: all
   // batches of one count of waves per CU get the same plans, the largest of them the largest grid (tests/test_launch_plans_cpu.py checks
   // both statements on dfs_choose and dfs_geometry) -- so one setup per class, both
   // algorithms, both precisions, both layouts, and the fp32 fused pair walk of mh_rnea_aba_f32 (batches from 8192 configurations on).
   // Largest class first: the workspace is allocated once, at its final size, where it can be.
   size_t dfs_bytes = 0;
   if (m->use_dfs)
   {
      const long cus = m->cu_count, classes = (groups_of(max_batch) + cus - 1) / cus;
      for (long wpc = classes; wpc >= 1; wpc--)
      {
         const int64_t B = std::min<int64_t>(max_batch, (int64_t)wpc * cus * 64);
         for (int aos = 0; aos < 2; aos++)
         {
            DfsSetup S{};
            for (Algo algo : {ALGO_RNEA, ALGO_ABA})
            {
               if ((st = dfs_setup<double>(algo, m, B, aos != 0, false, S)) != MH_OK)
                  return st;
               if ((st = dfs_setup<float>(algo, m, B, aos != 0, false, S)) != MH_OK)
                  return st;
            }
            if (m->use_dfs_pair && auto_transpose(m, B) && (st = dfs_setup<float>(ALGO_ABA, m, B, aos != 0, true, S)) != MH_OK)
               return st;
         }
      }
   }
   if (m->split_rt.usable) // the run-time tree split: one workspace block per workgroup
      dfs_bytes = std::max(dfs_bytes, split_rt_ws_bytes(m->split_rt.slots, split_rt_grid(m->cu_count, max_batch, 2), sizeof(double)));
   if (dfs_bytes > 0)
      st = ensure_bytes(m->ws, dfs_bytes);
   if (st == MH_OK && groups_of(max_batch) <= (long)m->cu_count)
      st = ensure_bytes(m->ws_pair, m->ws.bytes);
   // round 3's plans: the bias-split launches (their scratch for the largest batch they serve: two jobs on every group of 64 within the
   // CUs), the one-launch pair of the run-time tree split (twice the workgroups of a single call), the shared transposed copies of
   // mh_rnea_aba_f32 -- a call right after mh_reserve may be captured into a graph, where an allocation is an error
   if (st == MH_OK && m->spec.launch_zv && m->use_zv)
   {
      st = zv_prepare(m, std::min<int64_t>(max_batch, m->use_zv == 2 ? max_batch : 32L * m->cu_count), nullptr);
      if (st == MH_OK)
         HIP_TRY(hipStreamSynchronize(nullptr)); // the flags are zero before any stream's first launch looks at them
   }
   if (st == MH_OK && zvb_ok(m, max_batch, false) && !zvf_ok(m, max_batch, false))
   { // the two-launch forward dynamics of device-filling batches (models without the fused kernel): bias rows and (cos, sin) pairs
      st = ensure_bytes(m->zv_tau, (size_t)max_batch * m->nv * sizeof(double));
      if (st == MH_OK)
         st = ensure_bytes(m->zvb_cs, std::max<size_t>(1, (size_t)m->spec.zvb_cs_rows()) * (size_t)(groups_of(max_batch) * 64) * sizeof(double));
   }
   if (st == MH_OK && m->split_rt.usable) // the pair call's grid
      st = ensure_bytes(m->ws, split_rt_ws_bytes(m->split_rt.slots, std::min<long>(2 * groups_of(max_batch), (long)m->cu_count), sizeof(double)));
   if (st == MH_OK && transposed && m->use_dfs)
      st = ensure_bytes(m->tr_pair, (size_t)max_batch * ((size_t)m->nq + 5 * (size_t)m->nv) * sizeof(float));
   return st;
}

mh_status mh_rnea_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                      const double *f_ext, const mh_options *opts, double *tau_out)
{
   return launch<double>(ALGO_RNEA, model, B, q, qd, qdd, gravity, f_ext, opts, tau_out);
}
mh_status mh_aba_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                     const double *f_ext, const mh_options *opts, double *qdd_out)
{
   return launch<double>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, opts, qdd_out);
}
mh_status mh_crba_f64(mh_model_t model, int64_t B, const double *q, const mh_options *opts, double *H_out)
{
   return launch<double>(ALGO_CRBA, model, B, q, nullptr, nullptr, nullptr, nullptr, opts, H_out);
}
mh_status mh_regressor_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                           const mh_options *opts, int32_t first_moment_columns, double *Y_out)
{
   return regressor_impl<double>(model, B, q, qd, qdd, gravity, opts, first_moment_columns, Y_out);
}
mh_status mh_regressor_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                           const mh_options *opts, int32_t first_moment_columns, float *Y_out)
{
   return regressor_impl<float>(model, B, q, qd, qdd, gravity, opts, first_moment_columns, Y_out);
}
mh_status mh_crba_coriolis_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const mh_options *opts, double *H_out, double *C_out)
{
   return coriolis_impl<double>(model, B, q, qd, opts, H_out, C_out);
}
mh_status mh_crba_coriolis_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const mh_options *opts, float *H_out, float *C_out)
{
   return coriolis_impl<float>(model, B, q, qd, opts, H_out, C_out);
}
mh_status mh_centroidal_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double frame[12], int32_t frame_mode,
                            const mh_options *opts, double *A_out, double *b_out, double *com_out)
{
   return centroidal_impl<double>(model, B, q, qd, frame, frame_mode, opts, A_out, b_out, com_out);
}
mh_status mh_centroidal_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const double frame[12], int32_t frame_mode,
                            const mh_options *opts, float *A_out, float *b_out, float *com_out)
{
   return centroidal_impl<float>(model, B, q, qd, frame, frame_mode, opts, A_out, b_out, com_out);
}
mh_status mh_gravity_gradient_f64(mh_model_t model, int64_t B, const double *q, const double gravity[3], const double *f_ext,
                                  const mh_options *opts, double *tau_out, double *grad_out)
{
   return gravity_gradient_impl<double>(model, B, q, gravity, f_ext, opts, tau_out, grad_out);
}
mh_status mh_gravity_gradient_f32(mh_model_t model, int64_t B, const float *q, const double gravity[3], const float *f_ext, const mh_options *opts,
                                  float *tau_out, float *grad_out)
{
   return gravity_gradient_impl<float>(model, B, q, gravity, f_ext, opts, tau_out, grad_out);
}
mh_status mh_body_poses_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                            const mh_options *opts, double *pose_out)
{
   return kinematics_impl<double>("mh_body_poses_f64", false, model, B, q, nullptr, n_targets, nullptr, target_joints, target_poses, opts, pose_out, nullptr, nullptr);
}
mh_status mh_body_poses_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                            const mh_options *opts, float *pose_out)
{
   return kinematics_impl<float>("mh_body_poses_f32", false, model, B, q, nullptr, n_targets, nullptr, target_joints, target_poses, opts, pose_out, nullptr, nullptr);
}
mh_status mh_geometric_jacobian_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets, const int32_t *base_joints,
                                    const int32_t *target_joints, const double *target_poses, const mh_options *opts, double *J_out, double *conv_out)
{
   return kinematics_impl<double>("mh_geometric_jacobian_f64", true, model, B, q, qd, n_targets, base_joints, target_joints, target_poses, opts, nullptr, J_out,
                                  conv_out);
}
mh_status mh_geometric_jacobian_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets, const int32_t *base_joints,
                                    const int32_t *target_joints, const double *target_poses, const mh_options *opts, float *J_out, float *conv_out)
{
   return kinematics_impl<float>("mh_geometric_jacobian_f32", true, model, B, q, qd, n_targets, base_joints, target_joints, target_poses, opts, nullptr, J_out,
                                 conv_out);
}
mh_status mh_body_poses_vjp_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                const double *g_pose, const mh_options *opts, double *gq_out)
{
   return kinematics_vjp_impl<double>("mh_body_poses_vjp_f64", false, model, B, q, n_targets, nullptr, target_joints, target_poses, g_pose, opts, gq_out);
}
mh_status mh_body_poses_vjp_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                const float *g_pose, const mh_options *opts, float *gq_out)
{
   return kinematics_vjp_impl<float>("mh_body_poses_vjp_f32", false, model, B, q, n_targets, nullptr, target_joints, target_poses, g_pose, opts, gq_out);
}
mh_status mh_jacobian_transpose_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *base_joints, const int32_t *target_joints,
                                    const double *target_poses, const double *wrench, const mh_options *opts, double *tau_out)
{
   return kinematics_vjp_impl<double>("mh_jacobian_transpose_f64", true, model, B, q, n_targets, base_joints, target_joints, target_poses, wrench, opts, tau_out);
}
mh_status mh_jacobian_transpose_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *base_joints, const int32_t *target_joints,
                                    const double *target_poses, const float *wrench, const mh_options *opts, float *tau_out)
{
   return kinematics_vjp_impl<float>("mh_jacobian_transpose_f32", true, model, B, q, n_targets, base_joints, target_joints, target_poses, wrench, opts, tau_out);
}
mh_status mh_apparent_inertia_inverse_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *target_joints,
                                          const double *target_poses, int32_t blocks, const mh_options *opts, double *W_out)
{
   return apparent_inertia_impl<double>(model, B, q, n_targets, target_joints, target_poses, blocks, opts, W_out);
}
mh_status mh_apparent_inertia_inverse_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *target_joints,
                                          const double *target_poses, int32_t blocks, const mh_options *opts, float *W_out)
{
   return apparent_inertia_impl<float>(model, B, q, n_targets, target_joints, target_poses, blocks, opts, W_out);
}
mh_status mh_mass_matrix_inverse_f64(mh_model_t model, int64_t B, const double *q, int32_t n_columns, const int32_t *columns,
                                     const mh_options *opts, double *Hinv_out)
{
   return mass_matrix_inverse_impl<double>(model, B, q, n_columns, columns, opts, Hinv_out);
}
mh_status mh_mass_matrix_inverse_f32(mh_model_t model, int64_t B, const float *q, int32_t n_columns, const int32_t *columns,
                                     const mh_options *opts, float *Hinv_out)
{
   return mass_matrix_inverse_impl<float>(model, B, q, n_columns, columns, opts, Hinv_out);
}
mh_status mh_integrate_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *qdd, const mh_options *opts,
                           double *q_out, double *qd_out, double *qdd_out)
{
   return integrate_impl<double>(model, B, dt, q, qd, qdd, opts, q_out, qd_out, qdd_out);
}
mh_status mh_aba_integrate_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                               const double gravity[3], const double *f_ext, const mh_options *opts_in, double *qdd_out, double *q_next,
                               double *qd_next)
{
   mh_options o;
   mh_status st0 = begin_call(model, B, opts_in, o);
   if (st0 != MH_OK)
      return st0;
   if (B > 0 && (!q || !qd || !tau || !qdd_out || !q_next || !qd_next || (!gravity && !o.use_root_acceleration)))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   if (nan_bits(dt))
      return fail(MH_ERR_INVALID_ARGUMENT, "dt is NaN");
   const mh_options *opts = &o;
   if (B > 0)
   { // the new state may replace the old one; qdd_out is read again by the step, after the new state of other rows may have been written
      const size_t bq = (size_t)B * model->nq * sizeof(double), bv = (size_t)B * model->nv * sizeof(double);
      const InRange ins[4] = {{"q", q, bq}, {"qd", qd, bv}, {"tau", tau, bv}, {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(double)}};
      const OutRange outs[3] = {{"qdd_out", qdd_out, bv, 0u}, {"q_next", q_next, bq, 1u}, {"qd_next", qd_next, bv, 2u}};
      if (const mh_status sa = check_aliasing("mh_aba_integrate_f64", ins, 4, outs, 3); sa != MH_OK)
         return sa;
   }
   bool stepped = false;
   LaunchExtras<double> x;
   x.dt = dt, x.q_next = q_next, x.qd_next = qd_next, x.stepped = &stepped;
   mh_status st = launch<double>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, opts, qdd_out, x);
   if (st != MH_OK || stepped || B == 0)
      return st;
   return mh_integrate_f64(model, B, dt, q, qd, qdd_out, opts, q_next, qd_next, nullptr);
}
mh_status mh_integrate_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *qdd, const mh_options *opts,
                           float *q_out, float *qd_out, float *qdd_out)
{
   return integrate_impl<float>(model, B, dt, q, qd, qdd, opts, q_out, qd_out, qdd_out);
}
mh_status mh_rnea_bodies_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                             const double *f_ext, const mh_options *opts, double *tau_out, double *body_acc_out, double *body_twist_out)
{
   return launch<double>(ALGO_RNEA, model, B, q, qd, qdd, gravity, f_ext, opts, tau_out, body_outputs<double>(body_acc_out, body_twist_out));
}
mh_status mh_aba_bodies_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                            const double *f_ext, const mh_options *opts, double *qdd_out, double *body_acc_out, double *body_twist_out)
{
   return launch<double>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, opts, qdd_out, body_outputs<double>(body_acc_out, body_twist_out));
}
mh_status mh_rnea_joint_wrenches_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                                     const double *f_ext, const mh_options *opts, double *tau_out, double *joint_wrench_out)
{
   if (B > 0 && !joint_wrench_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "joint_wrench_out is NULL");
   return launch<double>(ALGO_RNEA, model, B, q, qd, qdd, gravity, f_ext, opts, tau_out, joint_wrenches(joint_wrench_out));
}
mh_status mh_aba_joint_wrenches_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                    const double *f_ext, const mh_options *opts, double *qdd_out, double *joint_wrench_out)
{
   if (B > 0 && !joint_wrench_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "joint_wrench_out is NULL");
   // the scratch below belongs to the CONTEXT of the call: resolve it before anything mutable is touched (launch() does so for itself only)
   mh_options o;
   mh_status st = begin_call(model, B, opts, o);
   if (st != MH_OK)
      return st;
   if (B > 0)
   { // before the first launch: the second one reads q, qd, f_ext and qdd_out again while it writes the wrenches
      const size_t bv = (size_t)B * model->nv * sizeof(double), bf = (size_t)B * model->n * 6 * sizeof(double);
      const InRange ins[4] = {{"q", q, (size_t)B * model->nq * sizeof(double)}, {"qd", qd, bv}, {"tau", tau, bv}, {"f_ext", f_ext, bf}};
      // (so qdd_out may be tau, which the second launch does not read, and nothing else)
      const OutRange outs[2] = {{"qdd_out", qdd_out, bv, 4u}, {"joint_wrench_out", joint_wrench_out, bf, 0u}};
      if ((st = check_aliasing("mh_aba_joint_wrenches_f64", ins, 4, outs, 2)) != MH_OK)
         return st;
   }
   st = launch<double>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, &o, qdd_out);
   if (st != MH_OK || B == 0)
      return st;
   // ForwardDynamicsCalculator.getJointWrench (ForwardDynamicsCalculator.java:1330-1363) is a Newton-Euler sweep over the accelerations
   // forward dynamics has just produced: the RNEA kernel with its joint-wrench output, on the same stream; its efforts (= tau up to
   // rounding) go to scratch
   st = ensure_bytes(model->aux, (size_t)B * model->nv * sizeof(double));
   if (st != MH_OK)
      return st;
   return launch<double>(ALGO_RNEA, model, B, q, qd, qdd_out, gravity, f_ext, &o, (double *)model->aux.ptr, joint_wrenches(joint_wrench_out));
}
mh_status mh_relative_acceleration_f64(mh_model_t model, int64_t B, const double *q, const double *body_acc, const double *body_twist,
                                       const double gravity[3], int32_t n_pairs, const int32_t *base_joints, const int32_t *body_joints,
                                       const mh_options *opts_in, double *out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (n_pairs < 0)
      return fail(MH_ERR_BAD_DIMENSION, "negative number of pairs %d", n_pairs);
   if (B == 0 || n_pairs == 0)
      return MH_OK;
   if (!q || !body_acc || (!gravity && !opts.use_root_acceleration) || !base_joints || !body_joints || !out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / pair / output pointer");
   model->pairs_host.resize((size_t)n_pairs * 2);
   for (int k = 0; k < n_pairs; k++)
   {
      const int b1 = base_joints[k], b2 = body_joints[k];
      if (b1 < -1 || b1 >= model->n || b2 < -1 || b2 >= model->n)
         return fail(MH_ERR_INVALID_ARGUMENT, "pair %d names joint %d / %d (the model has %d joints; -1 = the root body)", k, b1, b2, model->n);
      model->pairs_host[2 * k] = b1 < 0 ? -1 : model->engine_of[b1];
      model->pairs_host[2 * k + 1] = b2 < 0 ? -1 : model->engine_of[b2];
   }
   st = ensure_bytes(model->pairs, model->pairs_host.size() * sizeof(int));
   if (st != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   HIP_TRY(hipMemcpyAsync(model->pairs.ptr, model->pairs_host.data(), model->pairs_host.size() * sizeof(int), hipMemcpyHostToDevice, stream));
   mh::RelArgs<double> A{};
   A.m = dev_model<double>(model);
   A.B = B;
   A.q = q, A.body_acc = body_acc, A.body_twist = opts.consider_coriolis ? body_twist : nullptr, A.out = out;
   A.pairs = (const int *)model->pairs.ptr, A.n_pairs = n_pairs;
   const bool soa = opts.layout == MH_LAYOUT_SOA;
   set_strides(A.q_bs, A.q_es, soa, B, model->nq);
   set_strides(A.f_bs, A.f_es, soa, B, (long)model->n * 6);
   set_strides(A.o_bs, A.o_es, soa, B, (long)n_pairs * 6);
   set_root_acceleration(A, opts, gravity);
   if (opts.consider_coriolis && !body_twist)
      return fail(MH_ERR_INVALID_ARGUMENT, "body_twist is NULL but velocities are considered (opts->consider_coriolis)");
   const int block = 64;
   const int grid = (int)std::max<long>(1, std::min<long>((B + block - 1) / block, (long)model->cu_count * 8));
   hipLaunchKernelGGL((mh::relative_acceleration_kernel<double>), dim3(grid), dim3(block), 0, stream, A);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}
mh_status mh_model_set_joint_source_modes(mh_model_t model, const int32_t *modes)
{
   if (!model)
      return fail(MH_ERR_INVALID_ARGUMENT, "model is NULL");
   int cur = 0;
   if (hipGetDevice(&cur) != hipSuccess || cur != model->device)
      return fail(MH_ERR_INVALID_ARGUMENT, "model lives on device %d, which is not the calling thread's device", model->device);
   {
      std::lock_guard<std::mutex> lock(g_context_mutex);
      if (model->parent || model->n_contexts > 0)
         return fail(MH_ERR_INVALID_ARGUMENT, "joint source modes are set on the model itself, before its contexts are created (%d exist)", model->parent ? 1 : model->n_contexts);
   }
   for (int e = 0; modes && e < model->n; e++)
      if (modes[e] != MH_EFFORT_SOURCE && modes[e] != MH_ACCELERATION_SOURCE)
         return fail(MH_ERR_INVALID_ARGUMENT, "joint %d: unknown source mode %d", e, modes[e]);
   int n_locked = 0;
   for (int e = 0; e < model->n; e++)
   {
      int *mi = &model->meta[(size_t)e * mh::MI_STRIDE];
      const bool lk = modes && modes[mi[mh::MI_EXT]] == MH_ACCELERATION_SOURCE;
      mi[mh::MI_FLAGS] = (mi[mh::MI_FLAGS] & ~mh::MF_LOCKED) | (lk ? mh::MF_LOCKED : 0);
      n_locked += lk;
   }
   HIP_TRY(hipDeviceSynchronize());
   HIP_TRY(hipMemcpy(model->d_meta, model->meta.data(), model->meta.size() * sizeof(int), hipMemcpyHostToDevice));
   dfs_plans_drop(model); // copies of the records
   model->n_locked = n_locked;
   return MH_OK;
}
int32_t mh_model_n_acceleration_sources(mh_model_t model) { return model ? model->n_locked : -1; }
mh_status mh_aba_locked_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *qdd_in,
                            const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out, double *tau_out)
{
   return aba_locked<double>(model, B, q, qd, tau, qdd_in, gravity, f_ext, opts, qdd_out, tau_out);
}
// The pair calls run their two algorithms side by side (or phase by phase in one workgroup): an output that overlaps an input of the OTHER
// algorithm would be read half-written.  (mh_rnea_* then mh_aba_* is the call sequence for in-place use.)
mh_status mh_rnea_aba_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *tau,
                          const double gravity[3], const double *f_ext, const mh_options *opts_in, double *tau_out, double *qdd_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !qdd || !tau || (!gravity && !opts.use_root_acceleration) || !tau_out || !qdd_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   {
      const size_t bq = (size_t)B * model->nq * sizeof(double), bv = (size_t)B * model->nv * sizeof(double);
      const InRange ins[4] = {{"q", q, bq}, {"qd", qd, bv}, {"qdd", qdd, bv}, {"tau", tau, bv}};
      const OutRange outs[2] = {{"tau_out", tau_out, bv, 0u}, {"qdd_out", qdd_out, bv, 0u}};
      if ((st = check_aliasing("mh_rnea_aba_f64", ins, 4, outs, 2)) != MH_OK)
         return st;
   }
   const long waves = groups_of(B);
   const bool fusable = model->n_locked == 0 && model->spec.launch_fused && model->use_spec && model->dense_maps && opts.layout == MH_LAYOUT_AOS
                        && opts.consider_coriolis && opts.consider_accelerations && 2 * waves <= (long)model->cu_count * kFusedFactor
                        && model->spec.fused_lds_bytes(model->nq, model->nv) <= 160 * 1024
                        // beyond one group per CU the fused forward-dynamics kernel behind mh_aba_f64 is worth more than one launch for both
                        // (humanoid: 43.1 against 56.6 us at 32 768, 40.0 against 45.5 at 24 576; profiles/r04_pair_call_rates.txt)
                        && !zvf_ok(model, B, false);
   // No fused kernel for this call (no code object, SoA, switches, ...).  While the batch leaves most of the device idle -- the
   // run-time-topology kernels put one wave per 64 configurations on it -- the two launches run SIDE BY SIDE: the ABA on a stream of the
   // model's own, forked from and joined back into the caller's stream with events, on a workspace of its own (humanoid without its code
   // object, B = 4096: 63 + 112 us one after the other, ~115 us together).
   auto two_calls = [&]() -> mh_status {
      hipStream_t s = (hipStream_t)opts.stream;
      // no code object would serve either call and the run-time tree split serves both: one launch, half the grid each
      const bool no_spec = !model->use_spec || !model->spec.launch_split || !model->spec.split_usable || !model->spec.split_usable();
      if (no_spec && model->split_rt.usable && model->n_locked == 0 && model->use_split_rt != 0 && 2 * waves <= (long)model->cu_count)
      {
         mh::Args<double> P = make_args<double>(model, B, opts, gravity);
         P.q = q, P.qd = qd, P.in3 = qdd, P.fext = f_ext, P.out = tau_out;
         P.in3b = tau, P.outb = qdd_out;
         return launch_split_rt<double>(ALGO_ABA, model, B, P, s, true);
      }
      if (waves > (long)model->cu_count) // measured: pays up to one wave per CU (profiles/r02_generic_pair_side_by_side.txt)
      {
         mh_status r = mh_rnea_f64(model, B, q, qd, qdd, gravity, f_ext, &opts, tau_out);
         return r != MH_OK ? r : mh_aba_f64(model, B, q, qd, tau, gravity, f_ext, &opts, qdd_out);
      }
      return side_by_side(
         model, opts, true, [&](const mh_options *o) { return mh_rnea_f64(model, B, q, qd, qdd, gravity, f_ext, o, tau_out); },
         [&](const mh_options *o) { return mh_aba_f64(model, B, q, qd, tau, gravity, f_ext, o, qdd_out); });
   };
   // Device-filling batches: the fused forward-dynamics kernel computes tau too (its inverse-dynamics phase has h, one more walk without
   // velocities adds M(q) qdd of the caller's accelerations: mh_zv_kernels.h, ZvfDelta) -- one launch instead of the inverse dynamics'
   // own (humanoid, 262 144 configurations: 254 us for the two).  MH_ZVF_PAIR=0: the two launches.
   if (model->n_locked == 0 && model->use_spec && model->use_zvf_pair && opts.layout == MH_LAYOUT_AOS && opts.consider_coriolis && opts.consider_accelerations
       && zvf_ok(model, B, false) && model->spec.zvf_pair_usable && model->spec.zvf_pair_usable())
   {
      mh::Args<double> Z = make_args<double>(model, B, opts, gravity); // (AoS, both terms considered)
      Z.q = q, Z.qd = qd, Z.in3 = tau, Z.fext = f_ext, Z.out = qdd_out;
      Z.in3b = qdd, Z.outb = tau_out;
      const long groups = std::min<long>(waves, (long)model->cu_count * 2);
      if (spec_done(model->spec.launch_zvf(SPEC_IO_LDS | SPEC_IDENT, &Z, (int)groups, opts.stream), "fused forward + inverse dynamics failed to launch", st))
         return st;
   }
   if (!fusable)
      return two_calls();
   mh::Args<double> A = make_args<double>(model, B, opts, gravity); // (AoS, both terms considered)
   A.q = q, A.qd = qd, A.in3 = qdd, A.fext = f_ext, A.out = tau_out;
   A.in3b = tau, A.outb = qdd_out;
   if (zv_ok(model, B, false, 3))
   { // three jobs in one launch: bias efforts | articulated inertias + bias fold | the inverse dynamics output (mh_zv_kernels.h)
      if ((st = zv_check_error(model)) != MH_OK)
         return st;
      bool done = false;
      if ((st = zv_launch(model, A, 3, (hipStream_t)opts.stream, done)) != MH_OK || done)
         return st;
   }
   if (split_ok(model, 2, B, false))
   {
      if (spec_done(model->spec.launch_split(2, split_flags(model, 2, false), &A, (int)waves, opts.stream), "fused tree-split kernel launch failed", st))
         return st;
      return two_calls(); // not in this code object (fast build)
   }
   if (!model->spec.supports(1, SPEC_ST_LDS | (model->ident_maps ? SPEC_IDENT : 0)))
   // no whole-tree ABA in this code object (trees with a tree-split form) and the tree-split launch was ruled out: two calls
      return two_calls();
   if (spec_done(model->spec.launch_fused(model->ident_maps ? SPEC_IDENT : 0, &A, (int)waves, opts.stream), "fused kernel launch failed", st))
      return st;
   return two_calls();
}
mh_status mh_rnea_crba_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                           const double *f_ext, const mh_options *opts_in, double *tau_out, double *H_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !qdd || (!gravity && !opts.use_root_acceleration) || !tau_out || !H_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   { // the mass matrix reads q while the inverse dynamics writes tau_out: tau_out may be qd or qdd, never q; H_out is apart from everything
      const size_t bv = (size_t)B * model->nv * sizeof(double);
      const InRange ins[4] = {{"q", q, (size_t)B * model->nq * sizeof(double)}, {"qd", qd, bv}, {"qdd", qdd, bv},
                              {"f_ext", f_ext, (size_t)B * model->n * 6 * sizeof(double)}};
      const OutRange outs[2] = {{"tau_out", tau_out, bv, 6u}, {"H_out", H_out, bv * model->nv, 0u}};
      if ((st = check_aliasing("mh_rnea_crba_f64", ins, 4, outs, 2)) != MH_OK)
         return st;
   }
   hipStream_t s = (hipStream_t)opts.stream;
   const long groups = groups_of(B);
   // one launch: tree-split RNEA groups and tree-split CRBA groups side by side (code object with identity maps, AoS, no switches, no
   // external wrenches through this path; batches that leave room for both on the device)
   if (model->spec.launch_rnea_crba && model->use_spec && model->ident_maps && model->dense_maps && opts.layout == MH_LAYOUT_AOS
       && opts.consider_coriolis && opts.consider_accelerations && model->use_split != 0 && model->spec.split_usable && model->spec.split_usable()
       && model->spec.crba_split_usable && model->spec.crba_split_usable() && groups <= (long)model->cu_count * 2)
   {
      mh::Args<double> A = make_args<double>(model, B, opts, gravity); // (AoS, both terms considered)
      A.q = q, A.qd = qd, A.in3 = qdd, A.fext = f_ext, A.out = tau_out;
      A.outb = H_out;
      // thin CRBA workgroups: its write-out is bound by the stores in flight per CU.  Every workgroup must be resident at once (the RNEA
      // groups would otherwise queue behind the CRBA's): one per CU, two where the thinner image leaves LDS for it (202 registers: two
      // waves per SIMD)
      auto resident = [&](int l) {
         const long lds = model->spec.rnea_crba_lds_bytes ? model->spec.rnea_crba_lds_bytes(l, model->nq, model->nv) : 160 * 1024;
         return (long)model->cu_count * (2 * lds <= 160 * 1024 ? 2 : 1);
      };
      int lpg = 64;
      while (lpg > 16 && (B + lpg / 2 - 1) / (lpg / 2) + groups <= resident(lpg / 2))
         lpg /= 2;
      // ... and where the CUs the RNEA groups leave can take one CRBA workgroup each, the width that does exactly that: a workgroup that
      // shares its CU's SIMDs is the launch's last (humanoid, 4 096: 22 configurations in 187 workgroups beside the 64 RNEA groups 17.4 us,
      // 16 in 256: 18.0, 20 in 205: 19.0, 24: 18.7 -- profiles/r04_rnea_crba_lpg.txt)
      if (groups < (long)model->cu_count)
      {
         const long free_cus = (long)model->cu_count - groups;
         const long fit = (B + free_cus - 1) / free_cus;
         if (fit >= 16 && fit <= 64 && fit > lpg)
            lpg = (int)fit;
      }
      const long ng = std::min<long>((B + lpg - 1) / lpg, (long)model->cu_count * 2);
      if (spec_done(model->spec.launch_rnea_crba(&A, (int)groups, (int)ng, lpg, (void *)s), "fused RNEA + CRBA launch failed", st))
         return st;
   }
   // two launches; side by side while the batch leaves most of the device idle (the CRBA on the model's own stream; it needs no workspace
   // of the RNEA's kind when a code object serves it, and gets its own otherwise)
   if (groups > (long)model->cu_count)
   {
      st = mh_rnea_f64(model, B, q, qd, qdd, gravity, f_ext, &opts, tau_out);
      return st != MH_OK ? st : mh_crba_f64(model, B, q, &opts, H_out);
   }
   return side_by_side(
      model, opts, false, [&](const mh_options *o) { return mh_rnea_f64(model, B, q, qd, qdd, gravity, f_ext, o, tau_out); },
      [&](const mh_options *o) { return mh_crba_f64(model, B, q, o, H_out); });
}
mh_status mh_rnea_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                      const float *f_ext, const mh_options *opts, float *tau_out)
{
   return launch<float>(ALGO_RNEA, model, B, q, qd, qdd, gravity, f_ext, opts, tau_out);
}
mh_status mh_aba_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                     const float *f_ext, const mh_options *opts, float *qdd_out)
{
   return launch<float>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, opts, qdd_out);
}
mh_status mh_crba_f32(mh_model_t model, int64_t B, const float *q, const mh_options *opts, float *H_out)
{
   return launch<float>(ALGO_CRBA, model, B, q, nullptr, nullptr, nullptr, nullptr, opts, H_out);
}
// tau_out = RNEA(q, qd, qdd) and qdd_out = ABA(q, qd, tau) of the same configurations, fp32 (BASELINE.json configs[4]: both per step on
// the 128-body tree).  Where the forward dynamics of a big AoS batch would go through transposed scratch copies anyway (launch<T>), the
// copies of q and qd are made ONCE and serve both algorithms -- the inverse dynamics then runs on SoA strides instead of reading its
// rows through LDS windows (468 against 742 us at B = 131 072 on that tree) -- and both results are transposed back.  Same numbers as
// mh_rnea_f32 followed by mh_aba_f32 (the two layouts of the depth-first kernels agree bit for bit).
mh_status mh_rnea_aba_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *tau,
                          const double gravity[3], const float *f_ext, const mh_options *opts_in, float *tau_out, float *qdd_out)
{
   if (model && B > 0 && q && qd && qdd && tau && tau_out && qdd_out)
   {
      const size_t bq = (size_t)B * model->nq * sizeof(float), bv = (size_t)B * model->nv * sizeof(float);
      const InRange ins[4] = {{"q", q, bq}, {"qd", qd, bv}, {"qdd", qdd, bv}, {"tau", tau, bv}};
      const OutRange outs[2] = {{"tau_out", tau_out, bv, 0u}, {"qdd_out", qdd_out, bv, 0u}};
      if (const mh_status sa = check_aliasing("mh_rnea_aba_f32", ins, 4, outs, 2); sa != MH_OK)
         return sa;
   }
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts); // (the two single calls below check again, on the context's copy)
   if (st != MH_OK)
      return st;
   const bool big = q && qd && qdd && tau && tau_out && qdd_out && !f_ext && model->use_dfs && model->n_locked == 0 && model->use_transpose < 0
                    && auto_transpose(model, B) && opts.consider_coriolis && opts.consider_accelerations;
   const bool shared = big && opts.layout == MH_LAYOUT_AOS;
   // ONE walk for both (round 5; mh_dfs_kernels.h: aba_dfs_kernel<.., PAIR>) unless a run-time tree split or a code object serves the model
   // (small / specialised models hardly get here: 8192 configurations of >= 64 state entries); MH_DFS_PAIR=0 keeps the two launches
   // ... and unless the two single walks, which may keep twelve waves per CU resident where the pair walk keeps eight (dfs_choose), need so
   // many fewer rounds that they win: together they take 1.25 x the pair walk's time at equal occupancy, a round of twelve 1.32 x a round
   // of eight -- which leaves the batches of nine to twelve waves per CU (196 608 configurations: 1.82 against 2.11 ms)
   bool rounds_favour_two = false;
   if (big)
   {
      const long wpc = (groups_of(B) + model->cu_count - 1) / model->cu_count, r8 = (wpc + 7) / 8, r12 = (wpc + 11) / 12;
      const long two = (r12 * 132 < r8 * 100 ? r12 * 132 : r8 * 100) * 125; // (x 1e4)
      rounds_favour_two = two < r8 * 10000;
   }
   const bool fused = big && model->use_dfs_pair && !rounds_favour_two && !(model->spec.handle && model->use_spec)
                      && !(model->split_rt.usable && (model->use_split_rt == 1 || groups_of(B) <= (long)model->cu_count * 2));
   // the walk on SoA rows (the caller's, or the transposed copies): both terms considered
   auto fused_walk = [&](const float *sq, const float *sqd, const float *sqdd, const float *stau, float *o1, float *o2) -> mh_status {
      mh_options so = opts;
      so.layout = MH_LAYOUT_SOA;
      mh::Args<float> A = make_args<float>(model, B, so, gravity);
      A.q = sq, A.qd = sqd, A.in3 = sqdd, A.out = o1, A.in3b = stau, A.outb = o2;
      const mh_status r = launch_dfs<float>(ALGO_ABA, model, B, A, (hipStream_t)opts.stream, true);
      if (r == MH_OK)
         HIP_TRY(hipGetLastError());
      return r;
   };
   if (fused && opts.layout == MH_LAYOUT_SOA)
   { // SoA matrices: the walk reads and writes the caller's buffers
      if (!gravity && !opts.use_root_acceleration)
         return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
      return fused_walk(q, qd, qdd, tau, tau_out, qdd_out);
   }
   if (!shared)
   {
      const mh_status r = mh_rnea_f32(model, B, q, qd, qdd, gravity, f_ext, &opts, tau_out);
      return r != MH_OK ? r : mh_aba_f32(model, B, q, qd, tau, gravity, f_ext, &opts, qdd_out);
   }
   if (!gravity && !opts.use_root_acceleration)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   const size_t nq = model->nq, nv = model->nv, Bz = (size_t)B;
   st = ensure_bytes(model->tr_pair, Bz * (nq + 5 * nv) * sizeof(float));
   if (st != MH_OK)
      return st;
   float *t_q = (float *)model->tr_pair.ptr, *t_qd = t_q + Bz * nq, *t_qdd = t_qd + Bz * nv, *t_tau = t_qdd + Bz * nv, *t_o1 = t_tau + Bz * nv,
         *t_o2 = t_o1 + Bz * nv;
   hipStream_t stream = (hipStream_t)opts.stream;
   mh::transpose_rows<float>(q, t_q, (long)B, (long)nq, true, stream);
   mh::transpose_rows<float>(qd, t_qd, (long)B, (long)nv, true, stream);
   mh::transpose_rows<float>(qdd, t_qdd, (long)B, (long)nv, true, stream);
   mh::transpose_rows<float>(tau, t_tau, (long)B, (long)nv, true, stream);
   HIP_TRY(hipGetLastError());
   mh_options so = opts;
   so.layout = MH_LAYOUT_SOA;
   if (fused)
      st = fused_walk(t_q, t_qd, t_qdd, t_tau, t_o1, t_o2);
   else
   {
      st = launch<float>(ALGO_RNEA, model, B, t_q, t_qd, t_qdd, gravity, nullptr, &so, t_o1);
      if (st == MH_OK)
         st = launch<float>(ALGO_ABA, model, B, t_q, t_qd, t_tau, gravity, nullptr, &so, t_o2);
   }
   if (st != MH_OK)
      return st;
   mh::transpose_rows<float>(t_o1, tau_out, (long)B, (long)nv, false, stream);
   mh::transpose_rows<float>(t_o2, qdd_out, (long)B, (long)nv, false, stream);
   HIP_TRY(hipGetLastError());
   return MH_OK;
}

mh_status mh_rnea_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                           const double *f_ext, const mh_options *opts, double *tau_out)
{
   return launch_host<double>(ALGO_RNEA, model, B, q, qd, qdd, nullptr, gravity, f_ext, opts, tau_out, nullptr);
}
mh_status mh_aba_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                          const double *f_ext, const mh_options *opts, double *qdd_out)
{
   return launch_host<double>(ALGO_ABA, model, B, q, qd, tau, nullptr, gravity, f_ext, opts, qdd_out, nullptr);
}
mh_status mh_rnea_aba_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *tau,
                               const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out, double *qdd_out)
{
   return launch_host<double>(HOST_PAIR, model, B, q, qd, qdd, tau, gravity, f_ext, opts, tau_out, qdd_out);
}
mh_status mh_rnea_f32_host(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                           const float *f_ext, const mh_options *opts, float *tau_out)
{
   return launch_host<float>(ALGO_RNEA, model, B, q, qd, qdd, nullptr, gravity, f_ext, opts, tau_out, nullptr);
}
mh_status mh_aba_f32_host(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                          const float *f_ext, const mh_options *opts, float *qdd_out)
{
   return launch_host<float>(ALGO_ABA, model, B, q, qd, tau, nullptr, gravity, f_ext, opts, qdd_out, nullptr);
}
mh_status mh_crba_f32_host(mh_model_t model, int64_t B, const float *q, const mh_options *opts, float *H_out)
{
   return launch_host<float>(ALGO_CRBA, model, B, q, nullptr, nullptr, nullptr, nullptr, nullptr, opts, H_out, nullptr);
}
mh_status mh_rnea_bodies_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                             const float *f_ext, const mh_options *opts, float *tau_out, float *body_acc_out, float *body_twist_out)
{
   return launch<float>(ALGO_RNEA, model, B, q, qd, qdd, gravity, f_ext, opts, tau_out, body_outputs<float>(body_acc_out, body_twist_out));
}
mh_status mh_aba_bodies_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                            const float *f_ext, const mh_options *opts, float *qdd_out, float *body_acc_out, float *body_twist_out)
{
   return launch<float>(ALGO_ABA, model, B, q, qd, tau, gravity, f_ext, opts, qdd_out, body_outputs<float>(body_acc_out, body_twist_out));
}
mh_status mh_aba_locked_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *qdd_in,
                            const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out, float *tau_out)
{
   return aba_locked<float>(model, B, q, qd, tau, qdd_in, gravity, f_ext, opts, qdd_out, tau_out);
}
// ---- device memory for hosts without a HIP binding of their own (a Java shim keeps simulation state resident between steps with these)
mh_status mh_rnea_derivatives_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                                  const double *f_ext, const mh_options *opts, double *tau_out, double *dtau_dq_out, double *dtau_dqd_out)
{
   return rnea_derivatives_impl<double>(model, B, q, qd, qdd, gravity, f_ext, opts, tau_out, dtau_dq_out, dtau_dqd_out);
}
mh_status mh_rnea_derivatives_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                                  const float *f_ext, const mh_options *opts, float *tau_out, float *dtau_dq_out, float *dtau_dqd_out)
{
   return rnea_derivatives_impl<float>(model, B, q, qd, qdd, gravity, f_ext, opts, tau_out, dtau_dq_out, dtau_dqd_out);
}
mh_status mh_aba_constrained_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                 const double *f_ext, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                 const int32_t *target_rows, const int32_t *active, const double *a_des, double compliance, const mh_options *opts,
                                 double *qdd_out, double *lambda_out)
{
   return constrained_impl<double>(false, model, B, q, qd, tau, gravity, f_ext, n_targets, target_joints, target_poses, target_rows, active, a_des,
                                   compliance, opts, qdd_out, lambda_out);
}
mh_status mh_aba_constrained_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                                 const float *f_ext, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                 const int32_t *target_rows, const int32_t *active, const float *a_des, double compliance, const mh_options *opts,
                                 float *qdd_out, float *lambda_out)
{
   return constrained_impl<float>(false, model, B, q, qd, tau, gravity, f_ext, n_targets, target_joints, target_poses, target_rows, active, a_des,
                                  compliance, opts, qdd_out, lambda_out);
}
mh_status mh_aba_constrained_between_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                         const double *f_ext, int32_t n_targets, const int32_t *target_joints, const int32_t *base_joints,
                                         const double *target_poses, const int32_t *target_rows, const int32_t *active, const double *a_des,
                                         double compliance, const mh_options *opts, double *qdd_out, double *lambda_out)
{
   return constrained_impl<double>(false, model, B, q, qd, tau, gravity, f_ext, n_targets, target_joints, target_poses, target_rows, active, a_des,
                                   compliance, opts, qdd_out, lambda_out, true, base_joints);
}
mh_status mh_aba_constrained_between_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                                         const float *f_ext, int32_t n_targets, const int32_t *target_joints, const int32_t *base_joints,
                                         const double *target_poses, const int32_t *target_rows, const int32_t *active, const float *a_des,
                                         double compliance, const mh_options *opts, float *qdd_out, float *lambda_out)
{
   return constrained_impl<float>(false, model, B, q, qd, tau, gravity, f_ext, n_targets, target_joints, target_poses, target_rows, active, a_des,
                                  compliance, opts, qdd_out, lambda_out, true, base_joints);
}
mh_status mh_constraint_impulse_between_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets,
                                            const int32_t *target_joints, const int32_t *base_joints, const double *target_poses,
                                            const int32_t *target_rows, const int32_t *active, const double *v_des, double compliance,
                                            const mh_options *opts, double *qd_out, double *impulse_out)
{
   return constrained_impl<double>(true, model, B, q, qd, nullptr, nullptr, nullptr, n_targets, target_joints, target_poses, target_rows, active,
                                   v_des, compliance, opts, qd_out, impulse_out, true, base_joints);
}
mh_status mh_constraint_impulse_between_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets,
                                            const int32_t *target_joints, const int32_t *base_joints, const double *target_poses,
                                            const int32_t *target_rows, const int32_t *active, const float *v_des, double compliance,
                                            const mh_options *opts, float *qd_out, float *impulse_out)
{
   return constrained_impl<float>(true, model, B, q, qd, nullptr, nullptr, nullptr, n_targets, target_joints, target_poses, target_rows, active,
                                  v_des, compliance, opts, qd_out, impulse_out, true, base_joints);
}
mh_status mh_constraint_impulse_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets, const int32_t *target_joints,
                                    const double *target_poses, const int32_t *target_rows, const int32_t *active, const double *v_des,
                                    double compliance, const mh_options *opts, double *qd_out, double *impulse_out)
{
   return constrained_impl<double>(true, model, B, q, qd, nullptr, nullptr, nullptr, n_targets, target_joints, target_poses, target_rows, active,
                                   v_des, compliance, opts, qd_out, impulse_out);
}
mh_status mh_constraint_impulse_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets, const int32_t *target_joints,
                                    const double *target_poses, const int32_t *target_rows, const int32_t *active, const float *v_des,
                                    double compliance, const mh_options *opts, float *qd_out, float *impulse_out)
{
   return constrained_impl<float>(true, model, B, q, qd, nullptr, nullptr, nullptr, n_targets, target_joints, target_poses, target_rows, active,
                                  v_des, compliance, opts, qd_out, impulse_out);
}
mh_status mh_aba_derivatives_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                 const double *f_ext, const mh_options *opts, double *qdd_out, double *dqdd_dq_out, double *dqdd_dqd_out,
                                 double *Hinv_out)
{
   return aba_derivatives_impl<double>(model, B, q, qd, tau, gravity, f_ext, opts, qdd_out, dqdd_dq_out, dqdd_dqd_out, Hinv_out);
}
mh_status mh_aba_derivatives_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                                 const float *f_ext, const mh_options *opts, float *qdd_out, float *dqdd_dq_out, float *dqdd_dqd_out,
                                 float *Hinv_out)
{
   return aba_derivatives_impl<float>(model, B, q, qd, tau, gravity, f_ext, opts, qdd_out, dqdd_dq_out, dqdd_dqd_out, Hinv_out);
}
mh_status mh_contact_impulse_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets, const int32_t *target_joints,
                                 const double *target_poses, const double *mu, const double *normals, const int32_t *active, const double *v_normal,
                                 const double *impulse_init, double compliance, int32_t n_iterations, const mh_options *opts, double *qd_out,
                                 double *impulse_out, double *residual_out)
{
   return contact_impl<double>(model, B, q, qd, n_targets, target_joints, target_poses, mu, normals, active, v_normal, impulse_init, compliance,
                               n_iterations, opts, qd_out, impulse_out, residual_out);
}
mh_status mh_contact_impulse_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets, const int32_t *target_joints,
                                 const double *target_poses, const double *mu, const float *normals, const int32_t *active, const float *v_normal,
                                 const float *impulse_init, double compliance, int32_t n_iterations, const mh_options *opts, float *qd_out,
                                 float *impulse_out, float *residual_out)
{
   return contact_impl<float>(model, B, q, qd, n_targets, target_joints, target_poses, mu, normals, active, v_normal, impulse_init, compliance,
                              n_iterations, opts, qd_out, impulse_out, residual_out);
}
mh_status mh_contact_impulse_between_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets,
                                         const int32_t *target_joints, const int32_t *base_joints, const double *target_poses, const double *mu,
                                         const double *normals, const int32_t *active, const double *v_normal, const double *impulse_init,
                                         double compliance, int32_t n_iterations, const mh_options *opts, double *qd_out, double *impulse_out,
                                         double *residual_out)
{
   return contact_impl<double>(model, B, q, qd, n_targets, target_joints, target_poses, mu, normals, active, v_normal, impulse_init, compliance,
                               n_iterations, opts, qd_out, impulse_out, residual_out, true, base_joints);
}
mh_status mh_contact_impulse_between_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets,
                                         const int32_t *target_joints, const int32_t *base_joints, const double *target_poses, const double *mu,
                                         const float *normals, const int32_t *active, const float *v_normal, const float *impulse_init,
                                         double compliance, int32_t n_iterations, const mh_options *opts, float *qd_out, float *impulse_out,
                                         float *residual_out)
{
   return contact_impl<float>(model, B, q, qd, n_targets, target_joints, target_poses, mu, normals, active, v_normal, impulse_init, compliance,
                              n_iterations, opts, qd_out, impulse_out, residual_out, true, base_joints);
}
// not in include/mecano_hip.h: where the contact solve of this model (or context) reads S from now on -- -1 = contact_plan chooses,
// 0 = streamed, 1 = LDS-resident where it fits (tests/test_gpu_contact_dynamics.py holds the two to the same bits)
mh_status mh_internal_contact_path(mh_model_t model, int32_t path)
{
   if (!model || path < -1 || path > 1)
      return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_contact_path: model is NULL, or path is outside -1 ... 1");
   model->contact_path = path;
   return MH_OK;
}
mh_status mh_joint_limit_impulse_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_limits, const int32_t *limit_joints,
                                     const double *lower, const double *upper, double margin, double erp, const double *impulse_init,
                                     double compliance, int32_t n_iterations, const mh_options *opts, double *qd_out, double *impulse_out,
                                     double *residual_out)
{
   return limit_impl<double>(model, B, q, qd, n_limits, limit_joints, lower, upper, margin, erp, impulse_init, compliance, n_iterations, opts, qd_out,
                             impulse_out, residual_out);
}
mh_status mh_joint_limit_impulse_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_limits, const int32_t *limit_joints,
                                     const double *lower, const double *upper, double margin, double erp, const float *impulse_init,
                                     double compliance, int32_t n_iterations, const mh_options *opts, float *qd_out, float *impulse_out,
                                     float *residual_out)
{
   return limit_impl<float>(model, B, q, qd, n_limits, limit_joints, lower, upper, margin, erp, impulse_init, compliance, n_iterations, opts, qd_out,
                            impulse_out, residual_out);
}
// not in include/mecano_hip.h: where the joint-limit solve of this model (or context) reads S from now on -- -1 = limit_plan chooses,
// 0 = streamed, 1 = LDS-resident where it fits (tests/test_gpu_joint_limits.py holds the two to the same bits)
mh_status mh_internal_limit_path(mh_model_t model, int32_t path)
{
   if (!model || path < -1 || path > 1)
      return fail(MH_ERR_INVALID_ARGUMENT, "mh_internal_limit_path: model is NULL, or path is outside -1 ... 1");
   model->limit_path = path;
   return MH_OK;
}
mh_status mh_configuration_add_f64(mh_model_t model, int64_t B, const double *q, const double *dq, const mh_options *opts, double *q_out)
{
   return configuration_add_impl<double>(model, B, q, dq, opts, q_out);
}
mh_status mh_configuration_add_f32(mh_model_t model, int64_t B, const float *q, const float *dq, const mh_options *opts, float *q_out)
{
   return configuration_add_impl<float>(model, B, q, dq, opts, q_out);
}
mh_status mh_configuration_difference_f64(mh_model_t model, int64_t B, const double *q0, const double *q1, const mh_options *opts, double *dq_out)
{
   return configuration_difference_impl<double>(model, B, q0, q1, opts, dq_out);
}
mh_status mh_configuration_difference_f32(mh_model_t model, int64_t B, const float *q0, const float *q1, const mh_options *opts, float *dq_out)
{
   return configuration_difference_impl<float>(model, B, q0, q1, opts, dq_out);
}
mh_status mh_rnea_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                          const double *f_ext, const double *u, const mh_options *opts, double *gq_out, double *gqd_out, double *gqdd_out)
{
   return rnea_vjp_impl<double>(model, B, q, qd, qdd, gravity, f_ext, u, opts, gq_out, gqd_out, gqdd_out);
}
mh_status mh_rnea_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                          const float *f_ext, const float *u, const mh_options *opts, float *gq_out, float *gqd_out, float *gqdd_out)
{
   return rnea_vjp_impl<float>(model, B, q, qd, qdd, gravity, f_ext, u, opts, gq_out, gqd_out, gqdd_out);
}
mh_status mh_aba_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                         const double *f_ext, const double *w, const mh_options *opts, double *qdd_out, double *gq_out, double *gqd_out,
                         double *gtau_out)
{
   return aba_vjp_impl<double>(model, B, q, qd, tau, gravity, f_ext, w, opts, qdd_out, gq_out, gqd_out, gtau_out);
}
mh_status mh_aba_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                         const float *f_ext, const float *w, const mh_options *opts, float *qdd_out, float *gq_out, float *gqd_out, float *gtau_out)
{
   return aba_vjp_impl<float>(model, B, q, qd, tau, gravity, f_ext, w, opts, qdd_out, gq_out, gqd_out, gtau_out);
}
mh_status mh_aba_integrate_derivatives_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                                           const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out,
                                           double *q_next, double *qd_next, double *A_out, double *B_out)
{
   return step_derivatives_impl<double>(model, B, dt, q, qd, tau, gravity, f_ext, opts, qdd_out, q_next, qd_next, A_out, B_out);
}
mh_status mh_aba_integrate_derivatives_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *tau,
                                           const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out,
                                           float *q_next, float *qd_next, float *A_out, float *B_out)
{
   return step_derivatives_impl<float>(model, B, dt, q, qd, tau, gravity, f_ext, opts, qdd_out, q_next, qd_next, A_out, B_out);
}
mh_status mh_integrate_vjp_f64(mh_model_t model, int64_t B, double dt, const double *qd, const double *qdd, const double *gq_next,
                               const double *gqd_next, const mh_options *opts, double *gq_out, double *gqd_out, double *gqdd_out)
{
   return integrate_vjp_impl<double>(model, B, dt, qd, qdd, gq_next, gqd_next, opts, gq_out, gqd_out, gqdd_out);
}
mh_status mh_integrate_vjp_f32(mh_model_t model, int64_t B, double dt, const float *qd, const float *qdd, const float *gq_next,
                               const float *gqd_next, const mh_options *opts, float *gq_out, float *gqd_out, float *gqdd_out)
{
   return integrate_vjp_impl<float>(model, B, dt, qd, qdd, gq_next, gqd_next, opts, gq_out, gqd_out, gqdd_out);
}
mh_status mh_aba_integrate_vjp_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                                   const double gravity[3], const double *f_ext, const double *gq_next, const double *gqd_next,
                                   const mh_options *opts, double *qdd_out, double *gq_out, double *gqd_out, double *gtau_out)
{
   return step_vjp_impl<double>(model, B, dt, q, qd, tau, gravity, f_ext, gq_next, gqd_next, opts, qdd_out, gq_out, gqd_out, gtau_out);
}
mh_status mh_aba_integrate_vjp_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *tau,
                                   const double gravity[3], const float *f_ext, const float *gq_next, const float *gqd_next,
                                   const mh_options *opts, float *qdd_out, float *gq_out, float *gqd_out, float *gtau_out)
{
   return step_vjp_impl<float>(model, B, dt, q, qd, tau, gravity, f_ext, gq_next, gqd_next, opts, qdd_out, gq_out, gqd_out, gtau_out);
}
mh_status mh_rnea_jvp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                          const double *f_ext, const double *dq, const double *dqd, const double *dqdd, const mh_options *opts,
                          double *dtau_out)
{
   return rnea_jvp_impl<double>(model, B, q, qd, qdd, gravity, f_ext, dq, dqd, dqdd, opts, dtau_out);
}
mh_status mh_rnea_jvp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                          const float *f_ext, const float *dq, const float *dqd, const float *dqdd, const mh_options *opts,
                          float *dtau_out)
{
   return rnea_jvp_impl<float>(model, B, q, qd, qdd, gravity, f_ext, dq, dqd, dqdd, opts, dtau_out);
}
mh_status mh_aba_jvp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                         const double *f_ext, const double *dq, const double *dqd, const double *dtau, const mh_options *opts,
                         double *qdd_out, double *dqdd_out)
{
   return aba_jvp_impl<double>(model, B, q, qd, tau, gravity, f_ext, dq, dqd, dtau, opts, qdd_out, dqdd_out);
}
mh_status mh_aba_jvp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                         const float *f_ext, const float *dq, const float *dqd, const float *dtau, const mh_options *opts,
                         float *qdd_out, float *dqdd_out)
{
   return aba_jvp_impl<float>(model, B, q, qd, tau, gravity, f_ext, dq, dqd, dtau, opts, qdd_out, dqdd_out);
}
mh_status mh_integrate_jvp_f64(mh_model_t model, int64_t B, double dt, const double *qd, const double *qdd, const double *dq,
                               const double *dqd, const double *dqdd, const mh_options *opts, double *dq_next_out, double *dqd_next_out)
{
   return integrate_jvp_impl<double>(model, B, dt, qd, qdd, dq, dqd, dqdd, opts, dq_next_out, dqd_next_out);
}
mh_status mh_integrate_jvp_f32(mh_model_t model, int64_t B, double dt, const float *qd, const float *qdd, const float *dq,
                               const float *dqd, const float *dqdd, const mh_options *opts, float *dq_next_out, float *dqd_next_out)
{
   return integrate_jvp_impl<float>(model, B, dt, qd, qdd, dq, dqd, dqdd, opts, dq_next_out, dqd_next_out);
}
mh_status mh_aba_integrate_jvp_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                                   const double gravity[3], const double *f_ext, const double *dq, const double *dqd, const double *dtau,
                                   const mh_options *opts, double *qdd_out, double *dqdd_out, double *dq_next_out, double *dqd_next_out)
{
   return step_jvp_impl<double>(model, B, dt, q, qd, tau, gravity, f_ext, dq, dqd, dtau, opts, qdd_out, dqdd_out, dq_next_out, dqd_next_out);
}
mh_status mh_aba_integrate_jvp_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *tau,
                                   const double gravity[3], const float *f_ext, const float *dq, const float *dqd, const float *dtau,
                                   const mh_options *opts, float *qdd_out, float *dqdd_out, float *dq_next_out, float *dqd_next_out)
{
   return step_jvp_impl<float>(model, B, dt, q, qd, tau, gravity, f_ext, dq, dqd, dtau, opts, qdd_out, dqdd_out, dq_next_out, dqd_next_out);
}
mh_status mh_rnea_parameters_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *pi,
                                 const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out)
{
   return parameters_impl<double>(ALGO_RNEA, model, B, q, qd, qdd, pi, gravity, f_ext, opts, tau_out);
}
mh_status mh_rnea_parameters_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *pi,
                                 const double gravity[3], const float *f_ext, const mh_options *opts, float *tau_out)
{
   return parameters_impl<float>(ALGO_RNEA, model, B, q, qd, qdd, pi, gravity, f_ext, opts, tau_out);
}
mh_status mh_aba_parameters_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *pi,
                                const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out)
{
   return parameters_impl<double>(ALGO_ABA, model, B, q, qd, tau, pi, gravity, f_ext, opts, qdd_out);
}
mh_status mh_rnea_parameters_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *pi,
                                     const double gravity[3], const double *u, const mh_options *opts, double *gpi_out)
{
   return rnea_parameters_vjp_impl<double>(model, B, q, qd, qdd, pi, gravity, u, opts, gpi_out);
}
mh_status mh_rnea_parameters_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *pi,
                                     const double gravity[3], const float *u, const mh_options *opts, float *gpi_out)
{
   return rnea_parameters_vjp_impl<float>(model, B, q, qd, qdd, pi, gravity, u, opts, gpi_out);
}
mh_status mh_aba_parameters_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *pi,
                                    const double gravity[3], const double *f_ext, const double *w, const mh_options *opts, double *qdd_out,
                                    double *gtau_out, double *gpi_out)
{
   return aba_parameters_vjp_impl<double>(model, B, q, qd, tau, pi, gravity, f_ext, w, opts, qdd_out, gtau_out, gpi_out);
}
mh_status mh_aba_parameters_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *pi,
                                    const double gravity[3], const float *f_ext, const float *w, const mh_options *opts, float *qdd_out,
                                    float *gtau_out, float *gpi_out)
{
   return aba_parameters_vjp_impl<float>(model, B, q, qd, tau, pi, gravity, f_ext, w, opts, qdd_out, gtau_out, gpi_out);
}
mh_status mh_rnea_parameters_state_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *pi,
                                           const double gravity[3], const double *f_ext, const double *u, const mh_options *opts, double *gq_out,
                                           double *gqd_out, double *gqdd_out, double *gpi_out)
{
   return rnea_parameters_state_vjp_impl<double>(model, B, q, qd, qdd, pi, gravity, f_ext, u, opts, gq_out, gqd_out, gqdd_out, gpi_out);
}
mh_status mh_rnea_parameters_state_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *pi,
                                           const double gravity[3], const float *f_ext, const float *u, const mh_options *opts, float *gq_out,
                                           float *gqd_out, float *gqdd_out, float *gpi_out)
{
   return rnea_parameters_state_vjp_impl<float>(model, B, q, qd, qdd, pi, gravity, f_ext, u, opts, gq_out, gqd_out, gqdd_out, gpi_out);
}
mh_status mh_aba_parameters_state_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *pi,
                                          const double gravity[3], const double *f_ext, const double *w, const mh_options *opts, double *qdd_out,
                                          double *gq_out, double *gqd_out, double *gtau_out, double *gpi_out)
{
   return aba_parameters_state_vjp_impl<double>(model, B, q, qd, tau, pi, gravity, f_ext, w, opts, qdd_out, gq_out, gqd_out, gtau_out, gpi_out);
}
mh_status mh_aba_parameters_state_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *pi,
                                          const double gravity[3], const float *f_ext, const float *w, const mh_options *opts, float *qdd_out,
                                          float *gq_out, float *gqd_out, float *gtau_out, float *gpi_out)
{
   return aba_parameters_state_vjp_impl<float>(model, B, q, qd, tau, pi, gravity, f_ext, w, opts, qdd_out, gq_out, gqd_out, gtau_out, gpi_out);
}
mh_status mh_aba_parameters_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *pi,
                                const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out)
{
   return parameters_impl<float>(ALGO_ABA, model, B, q, qd, tau, pi, gravity, f_ext, opts, qdd_out);
}
mh_status mh_device_alloc(size_t bytes, void **ptr_out)
{
   if (!ptr_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "ptr_out is NULL");
   *ptr_out = nullptr;
   HIP_TRY(hipMalloc(ptr_out, bytes ? bytes : 1));
   return MH_OK;
}
mh_status mh_device_free(void *ptr)
{
   if (ptr)
      HIP_TRY(hipFree(ptr));
   return MH_OK;
}
mh_status mh_copy_to_device(void *dst_device, const void *src_host, size_t bytes, void *stream)
{
   if (bytes && (!dst_device || !src_host))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL pointer");
   HIP_TRY(hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
   return MH_OK;
}
mh_status mh_copy_to_host(void *dst_host, const void *src_device, size_t bytes, void *stream)
{
   if (bytes && (!dst_host || !src_device))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL pointer");
   HIP_TRY(hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
   return MH_OK;
}
mh_status mh_stream_synchronize(void *stream)
{
   HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
   return check_all_error_words(); // an inertia job that gave up waiting (mh_zv_kernels.h): reported here, not at the model's next call
}
mh_status mh_host_alloc(size_t bytes, void **ptr_out)
{
   if (!ptr_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "ptr_out is NULL");
   *ptr_out = nullptr;
   HIP_TRY(hipHostMalloc(ptr_out, bytes ? bytes : 1, hipHostMallocDefault));
   return MH_OK;
}
mh_status mh_host_free(void *ptr)
{
   if (ptr)
      HIP_TRY(hipHostFree(ptr));
   return MH_OK;
}
mh_status mh_host_register(void *ptr, size_t bytes)
{
   if (!ptr || !bytes)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL pointer / empty range");
   HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
   return MH_OK;
}
mh_status mh_host_unregister(void *ptr)
{
   if (ptr)
      HIP_TRY(hipHostUnregister(ptr));
   return MH_OK;
}
mh_status mh_crba_f64_host(mh_model_t model, int64_t B, const double *q, const mh_options *opts, double *H_out)
{
   return launch_host<double>(ALGO_CRBA, model, B, q, nullptr, nullptr, nullptr, nullptr, nullptr, opts, H_out, nullptr);
}

// ---- HIP-event timer
struct mh_timer
{
   hipEvent_t start, stop;
};
mh_status mh_crba_coriolis_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const mh_options *opts_in, double *H_out,
                                    double *C_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !qd || !H_out || !C_out)
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer");
   const size_t s_q = (size_t)B * model->nq, s_v = (size_t)B * model->nv, s_h = (size_t)B * model->nv * model->nv;
   st = ensure_bytes(model->stage, (s_q + s_v + 2 * s_h) * sizeof(double));
   if (st != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   double *d_q = (double *)model->stage.ptr, *d_qd = d_q + s_q, *d_H = d_qd + s_v, *d_C = d_H + s_h;
   HIP_TRY(hipMemcpyAsync(d_q, q, s_q * sizeof(double), hipMemcpyHostToDevice, stream));
   HIP_TRY(hipMemcpyAsync(d_qd, qd, s_v * sizeof(double), hipMemcpyHostToDevice, stream));
   st = coriolis_impl<double>(model, B, d_q, d_qd, &opts, d_H, d_C);
   if (st != MH_OK)
      return st;
   HIP_TRY(hipMemcpyAsync(H_out, d_H, s_h * sizeof(double), hipMemcpyDeviceToHost, stream));
   HIP_TRY(hipMemcpyAsync(C_out, d_C, s_h * sizeof(double), hipMemcpyDeviceToHost, stream));
   HIP_TRY(hipStreamSynchronize(stream));
   return MH_OK;
}
mh_status mh_centroidal_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double frame[12], int32_t frame_mode,
                                 const mh_options *opts_in, double *A_out, double *b_out, double *com_out)
{
   mh_options opts;
   mh_status st = begin_call(model, B, opts_in, opts);
   if (st != MH_OK)
      return st;
   if (B == 0)
      return MH_OK;
   if (!q || !A_out || (b_out && !qd))
      return fail(MH_ERR_INVALID_ARGUMENT, "NULL state / output pointer (the convective term needs qd)");
   const size_t s_q = (size_t)B * model->nq, s_v = (size_t)B * model->nv, s_a = (size_t)B * 6 * model->nv, s_b = (size_t)B * 6, s_c = (size_t)B * 3;
   st = ensure_bytes(model->stage, (s_q + s_v + s_a + s_b + s_c) * sizeof(double));
   if (st != MH_OK)
      return st;
   hipStream_t stream = (hipStream_t)opts.stream;
   double *d_q = (double *)model->stage.ptr, *d_qd = d_q + s_q, *d_A = d_qd + s_v, *d_b = d_A + s_a, *d_c = d_b + s_b;
   HIP_TRY(hipMemcpyAsync(d_q, q, s_q * sizeof(double), hipMemcpyHostToDevice, stream));
   if (qd)
      HIP_TRY(hipMemcpyAsync(d_qd, qd, s_v * sizeof(double), hipMemcpyHostToDevice, stream));
   st = centroidal_impl<double>(model, B, d_q, qd ? d_qd : nullptr, frame, frame_mode, &opts, d_A, b_out ? d_b : nullptr, com_out ? d_c : nullptr);
   if (st != MH_OK)
      return st;
   HIP_TRY(hipMemcpyAsync(A_out, d_A, s_a * sizeof(double), hipMemcpyDeviceToHost, stream));
   if (b_out)
      HIP_TRY(hipMemcpyAsync(b_out, d_b, s_b * sizeof(double), hipMemcpyDeviceToHost, stream));
   if (com_out)
      HIP_TRY(hipMemcpyAsync(com_out, d_c, s_c * sizeof(double), hipMemcpyDeviceToHost, stream));
   HIP_TRY(hipStreamSynchronize(stream));
   return MH_OK;
}

mh_status mh_timer_create(mh_timer_t *out)
{
   if (!out)
      return fail(MH_ERR_INVALID_ARGUMENT, "timer_out is NULL");
   mh_timer *t = new mh_timer();
   // timing only: without the system-scope fence (cache write-back) a default event performs when it becomes recorded -- measured on the
   // headline's regions of 20 steps: 8 us per region with default events (profiles/r04_region_overhead.txt)
   if (hipEventCreateWithFlags(&t->start, hipEventDisableSystemFence) != hipSuccess
       || hipEventCreateWithFlags(&t->stop, hipEventDisableSystemFence) != hipSuccess)
   {
      delete t;
      return fail(MH_ERR_NO_DEVICE, "cannot create HIP events");
   }
   *out = t;
   return MH_OK;
}
void mh_timer_destroy(mh_timer_t t)
{
   if (!t)
      return;
   (void)hipEventDestroy(t->start);
   (void)hipEventDestroy(t->stop);
   delete t;
}
mh_status mh_timer_start(mh_timer_t t, void *stream)
{
   if (!t)
      return fail(MH_ERR_INVALID_ARGUMENT, "timer is NULL");
   HIP_TRY(hipEventRecord(t->start, (hipStream_t)stream));
   return MH_OK;
}
mh_status mh_timer_stop(mh_timer_t t, void *stream)
{
   if (!t)
      return fail(MH_ERR_INVALID_ARGUMENT, "timer is NULL");
   HIP_TRY(hipEventRecord(t->stop, (hipStream_t)stream));
   return MH_OK;
}
mh_status mh_timer_elapsed_ms(mh_timer_t t, float *ms)
{
   if (!t || !ms)
      return fail(MH_ERR_INVALID_ARGUMENT, "timer / ms_out is NULL");
   HIP_TRY(hipEventSynchronize(t->stop));
   HIP_TRY(hipEventElapsedTime(ms, t->start, t->stop));
   return MH_OK;
}

} // extern "C"

// =================================================================================================== create-time self-check
// A topology-specialised code object is machine-generated straight-line code at the edge of the register file (open issues:
// one whole-tree ABA build of a 25-body tree returned wrong numbers).  So a freshly loaded object is not trusted: 197 seeded
// configurations (three full groups of 64 and a ragged one) go through every call the dispatcher can route to it -- RNEA, ABA, the fused
// pair, the fused simulation step, CRBA, the per-body variants, Coriolis and centroidal quantities, AoS and SoA, with the real CU count
// (small-batch plans) and with a pretended single CU (device-filling plans: global hand-over store, three-wave RNEA build) -- and through
// the run-time-topology kernels.  On disagreement the object is dropped and mh_model_kernel_variant says why; the model then runs on the
// run-time-topology kernels.  MH_SPEC_SELFCHECK=0 skips the check.
namespace
{
struct Lcg
{
   unsigned long long s;
   double u(double lo, double hi)
   {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      return lo + (hi - lo) * (double)(s >> 11) / 9007199254740992.0;
   }
};
enum CheckCase
{
   CK_RNEA,
   CK_ABA,
   CK_CRBA,
   CK_FUSED,
   CK_STEP,
   CK_BODIES_RNEA,
   CK_BODIES_ABA,
   CK_CORIOLIS,
   CK_CENTROIDAL,
   CK_COUNT
};
// fills the check's output buffer with the NaN pattern 0xFF..FF ON THE LAUNCH STREAM: the synchronous hipMemset was observed to be
// unordered against null-stream kernels of this process (results wiped after the kernel had written them, or never wiped), which showed up
// as intermittent refusals / acceptances
__global__ void __launch_bounds__(256) fill_nan_kernel(unsigned long long *p, size_t n)
{
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
      p[i] = ~0ull;
}
const char *const kCheckNames[CK_COUNT] = {"RNEA", "ABA", "CRBA", "fused RNEA+ABA", "ABA + integration step", "RNEA with per-body outputs",
                                           "ABA with per-body outputs", "mass + Coriolis matrix", "centroidal momentum"};
} // namespace

static void self_check_spec(mh_model *m)
{
   const int64_t B = 64 * 3 + 5;
   const size_t nq = m->nq, nv = m->nv, n = m->n;
   if (nv == 0)
      return;
   Lcg rng{0x9E3779B97F4A7C15ull ^ (unsigned long long)n};
   std::vector<double> q((size_t)B * nq, 0.0), qd((size_t)B * nv), qdd((size_t)B * nv), tau((size_t)B * nv);
   for (int64_t b = 0; b < B; b++)
      for (int e = 0; e < m->n; e++)
      {
         const int *mi = &m->meta[(size_t)e * mh::MI_STRIDE];
         const int t = mi[mh::MI_TYPE], *ci = &m->cfg_map[mi[mh::MI_CFG]];
         double *row = &q[(size_t)b * nq];
         if (t == MH_JOINT_REVOLUTE)
            row[ci[0]] = rng.u(-3.14159, 3.14159);
         else if (t == MH_JOINT_PRISMATIC)
            row[ci[0]] = rng.u(-1, 1);
         else if (t == MH_JOINT_SIXDOF || t == MH_JOINT_SPHERICAL)
         {
            double qt[4], nrm = 0;
            for (int k = 0; k < 4; k++)
               qt[k] = rng.u(-1, 1), nrm += qt[k] * qt[k];
            nrm = std::sqrt(nrm) + 1e-300;
            for (int k = 0; k < 4; k++)
               row[ci[k]] = qt[k] / nrm;
            for (int k = 4; k < joint_ncfg(t); k++)
               row[ci[k]] = rng.u(-1, 1);
         }
         else if (t == MH_JOINT_PLANAR)
            row[ci[0]] = rng.u(-3.14159, 3.14159), row[ci[1]] = rng.u(-1, 1), row[ci[2]] = rng.u(-1, 1);
      }
   for (size_t k = 0; k < (size_t)B * nv; k++)
      qd[k] = rng.u(-1, 1), qdd[k] = rng.u(-1, 1), tau[k] = rng.u(-1, 1);
   auto transposed = [&](const std::vector<double> &a, size_t cols) {
      std::vector<double> t(a.size());
      for (int64_t b = 0; b < B; b++)
         for (size_t c = 0; c < cols; c++)
            t[c * (size_t)B + (size_t)b] = a[(size_t)b * cols + c];
      return t;
   };
   const size_t out_doubles = (size_t)B * std::max<size_t>({2 * nv * nv, 6 * nv + 9, 2 * nv + 19 * n}) + 64;
   const size_t in_doubles = (size_t)B * (nq + 3 * nv);
   double *d_all = nullptr;
   if (hipMalloc((void **)&d_all, (2 * in_doubles + out_doubles) * sizeof(double)) != hipSuccess)
      return; // cannot check: keep the object (the allocation failure will surface in the first compute call anyway)
   double *d_in[2] = {d_all, d_all + in_doubles}, *d_out = d_all + 2 * in_doubles;
   for (int L = 0; L < 2; L++)
   {
      const std::vector<double> *src[4] = {&q, &qd, &qdd, &tau};
      const size_t cols[4] = {nq, nv, nv, nv};
      size_t ofs = 0;
      for (int k = 0; k < 4; k++)
      {
         const std::vector<double> t = L == 0 ? *src[k] : transposed(*src[k], cols[k]);
         (void)hipMemcpy(d_in[L] + ofs, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice);
         ofs += (size_t)B * cols[k];
      }
   }
   const double gravity[3] = {0.3, -0.2, -9.81};
   auto run = [&](int what, int L, size_t &used) -> mh_status {
      mh_options o;
      mh_options_default(&o);
      o.layout = L == 0 ? MH_LAYOUT_AOS : MH_LAYOUT_SOA;
      // a rotating, accelerating base: every plan starts its outward sweep from the full 6-D root acceleration
      o.use_root_acceleration = 1;
      const double root_acc[6] = {0.11, -0.07, 0.05, -0.3, 0.2, 9.81};
      for (int k = 0; k < 6; k++)
         o.root_acceleration[k] = root_acc[k];
      const double *dq = d_in[L], *dqd = dq + (size_t)B * nq, *dqdd = dqd + (size_t)B * nv, *dtau = dqdd + (size_t)B * nv;
      double *o1 = d_out, *o2 = o1 + (size_t)B * nv, *o3 = o2 + (size_t)B * std::max(nq, 6 * n);
      hipLaunchKernelGGL(fill_nan_kernel, dim3(64), dim3(256), 0, (hipStream_t) nullptr, (unsigned long long *)d_out, out_doubles);
      switch (what)
      {
         case CK_RNEA: used = (size_t)B * nv; return mh_rnea_f64(m, B, dq, dqd, dqdd, gravity, nullptr, &o, o1);
         case CK_ABA: used = (size_t)B * nv; return mh_aba_f64(m, B, dq, dqd, dtau, gravity, nullptr, &o, o1);
         case CK_CRBA: used = (size_t)B * nv * nv; return mh_crba_f64(m, B, dq, &o, o1);
         case CK_FUSED: used = 2 * (size_t)B * nv; return mh_rnea_aba_f64(m, B, dq, dqd, dqdd, dtau, gravity, nullptr, &o, o1, o2);
         case CK_STEP:
            used = (size_t)B * (nv + std::max(nq, 6 * n) + nv);
            return mh_aba_integrate_f64(m, B, 1.0e-3, dq, dqd, dtau, gravity, nullptr, &o, o1, o2, o3);
         case CK_BODIES_RNEA:
            used = (size_t)B * (nv + std::max(nq, 6 * n) + 6 * n);
            return mh_rnea_bodies_f64(m, B, dq, dqd, dqdd, gravity, nullptr, &o, o1, o2, o3);
         case CK_BODIES_ABA:
            used = (size_t)B * (nv + std::max(nq, 6 * n) + 6 * n);
            return mh_aba_bodies_f64(m, B, dq, dqd, dtau, gravity, nullptr, &o, o1, o2, o3);
         case CK_CORIOLIS: used = 2 * (size_t)B * nv * nv; return mh_crba_coriolis_f64(m, B, dq, dqd, &o, d_out, d_out + (size_t)B * nv * nv);
         case CK_CENTROIDAL:
            used = (size_t)B * (6 * nv + 9);
            return mh_centroidal_f64(m, B, dq, dqd, nullptr, MH_CENTROIDAL_FRAME_AT_COM, &o, d_out, d_out + (size_t)B * 6 * nv,
                                     d_out + (size_t)B * (6 * nv + 6));
      }
      return MH_OK;
   };
   const int real_cus = m->cu_count;
   static const char *const kPlanNames[5] = {"small-batch", "device-filling", "tree-split", "device-filling, two launches", "device-filling, one job"};
   const bool verbose = getenv("MH_SPEC_SELFCHECK_VERBOSE") != nullptr;
   std::vector<unsigned long long> ref, got; // raw words: see nan_word
   std::string failure;
   for (int what = 0; what < CK_COUNT && failure.empty(); what++)
      for (int L = 0; L < 2 && failure.empty(); L++)
      {
         if ((what == CK_FUSED || what == CK_STEP) && L == 1)
            continue; // AoS-only entry points
         size_t used = 0;
         m->use_spec = 0;
         mh_status st = run(what, L, used);
         (void)hipDeviceSynchronize();
         m->use_spec = 1;
         if (st != MH_OK)
            continue; // the run-time-topology kernels cannot serve this call either: nothing to compare
         ref.resize(used);
         (void)hipMemcpy(ref.data(), d_out, used * sizeof(double), hipMemcpyDeviceToHost);
         // plan 0: the real CU count; 1: a pretended single CU (device-filling plans); 2: the bias-split forward dynamics switched off
         // (the tree-split kernels it replaced still serve SoA calls, simulation steps and models with acceleration sources)
         // 3: a pretended single CU with the fused forward dynamics switched off (the one-job kernel's device-filling plan, plan 4, is what
         // serves SoA calls and simulation steps at those sizes)
         // 4: ... with the fused one-launch form switched off as well (plan 1 takes the fused kernel where the code object has it, plan 3 then
         // the two launches, plan 4 the one-job kernel)
         // (inverse dynamics: plan 1 takes the loop that requests rows ahead, plan 4 the tree-split kernel's own device-filling loop)
         const int zv_was = m->use_zv, zvb_was = m->use_zvb, zvf_was = m->use_zvf, ahead_was = m->use_rnea_ahead;
         const bool zv_plan = (what == CK_ABA || what == CK_FUSED) && L == 0 && zv_was && zv_ok(m, B, false, what == CK_FUSED ? 3 : 2);
         m->cu_count = 1;
         const bool fd_aos = (what == CK_ABA || what == CK_FUSED) && L == 0;
         const bool zvf_plan = fd_aos && zvf_was && zvf_ok(m, B, false), zvb_plan = fd_aos && zvb_was && zvb_ok(m, B, false);
         const bool ahead_plan = (what == CK_RNEA || what == CK_FUSED) && L == 0 && ahead_was && rnea_ahead_ok(m, B, false);
         m->cu_count = real_cus;
         for (int plan = 0; plan < 5 && failure.empty(); plan++)
         {
            if ((plan == 2 && !zv_plan) || (plan == 3 && !(zvf_plan && zvb_plan)) || (plan == 4 && !(zvf_plan || zvb_plan || ahead_plan)))
               continue;
            const int pretend = plan == 1 || plan >= 3 ? 1 : 0;
            m->cu_count = pretend ? 1 : real_cus;
            m->use_zv = plan == 2 ? 0 : zv_was;
            m->use_zvf = plan >= 3 ? 0 : zvf_was;
            m->use_zvb = plan == 4 ? 0 : zvb_was;
            m->use_rnea_ahead = plan >= 3 ? 0 : ahead_was;
            st = run(what, L, used);
            const hipError_t sync = hipDeviceSynchronize();
            m->cu_count = real_cus;
            m->use_zv = zv_was;
            m->use_zvb = zvb_was;
            m->use_zvf = zvf_was;
            m->use_rnea_ahead = ahead_was;
            if (st == MH_OK)
               st = zv_check_error(m);
            char buf[320];
            if (st != MH_OK || sync != hipSuccess)
            {
               snprintf(buf, sizeof buf, "%s (%s, %s plan) failed: %s", kCheckNames[what], L ? "SoA" : "AoS",
                        kPlanNames[plan], st != MH_OK ? g_err : hipGetErrorString(sync));
               failure = buf;
               break;
            }
            got.resize(used);
            (void)hipMemcpy(got.data(), d_out, used * sizeof(double), hipMemcpyDeviceToHost);
            double scale = 1.0, err = 0.0;
            bool nan_mismatch = false;
            size_t first_bad = 0;
            bool bad_is_unwritten = false;
            for (size_t k = 0; k < used; k++)
            {
               // bit tests, not x != x: this translation unit is built with -ffinite-math-only, under which the compiler folds NaN tests away
               const bool rn = nan_word(ref[k]), gn = nan_word(got[k]);
               if (rn != gn)
               {
                  if (!nan_mismatch)
                     first_bad = k, bad_is_unwritten = gn;
                  nan_mismatch = true;
               }
               else if (!rn)
               {
                  double rv, gv;
                  std::memcpy(&rv, &ref[k], sizeof rv), std::memcpy(&gv, &got[k], sizeof gv);
                  scale = std::max(scale, std::fabs(rv)), err = std::max(err, std::fabs(rv - gv));
               }
            }
            // forward dynamics divides by joint-space inertias: rounding differences between two exact evaluation orders are amplified by
            // their conditioning (1e-8 is what the parity tests grant ill-conditioned random trees); everything else is held to 1e-10
            const double tol = (what == CK_ABA || what == CK_FUSED || what == CK_STEP || what == CK_BODIES_ABA) ? 1.0e-8 : 1.0e-10;
            if (verbose)
               fprintf(stderr, "[mh self-check] %-28s %s %-14s  |diff| %.3e  |ref| %.3e  unwritten-mismatch %d (word %zu)\n", kCheckNames[what], L ? "SoA" : "AoS",
                       kPlanNames[plan], err, scale, (int)nan_mismatch, first_bad);
            if (nan_mismatch || err > tol * scale)
            {
               char where[96] = "";
               if (nan_mismatch)
                  snprintf(where, sizeof where, ", output word %zu %s", first_bad,
                           bad_is_unwritten ? "left unwritten" : "written although the run-time-topology kernels do not write it");
               snprintf(buf, sizeof buf, "%s (%s, %s plan) differs from the run-time-topology kernels by %.3e (|ref| <= %.3e%s)", kCheckNames[what],
                        L ? "SoA" : "AoS", kPlanNames[plan], err, scale, where);
               failure = buf;
            }
         }
      }
   (void)hipFree(d_all);
   if (!failure.empty())
   {
      dlclose(m->spec.handle);
      m->spec = SpecLib{};
      m->variant = "generic (code object topo:" + m->topo_key + " refused by the create-time self-check: " + failure + ")";
   }
}
