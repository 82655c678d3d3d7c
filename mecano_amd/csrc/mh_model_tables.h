// mh_model_tables.h -- what a model IS, compiled on the host from the caller's mh_model_desc: validation and the engine's joint order
// (plan_model), then every table the kernels read (compile_model -> ModelTables).  Pure host arithmetic: nothing here calls the HIP
// runtime, so the tables can be read -- and this code run under sanitizers -- on a machine without a device (mh_internal_model_table,
// tests/test_model_tables_cpu.py, tests/test_model_tables_sanitizers.py).  mh_api.hip uploads the tables (DeviceTables) and launches.
//
// Included by one translation unit of the library (mh_api.hip) and by stand-alone test programs: everything lives in an unnamed namespace.
#pragma once
#include "../../include/mecano_hip.h"
#include "mh_dfs_kernels.h"
#include "mh_response_kernels.h"
#include "mh_rnea_deriv_kernels.h"
#include "mh_params_kernels.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace
{
// the calling thread's last error text (mh_last_error): lives here so that plan_model and compile_model report as every entry point does
thread_local char g_err[512] = "";

mh_status fail(mh_status code, const char *fmt, ...)
{
   va_list ap;
   va_start(ap, fmt);
   vsnprintf(g_err, sizeof g_err, fmt, ap);
   va_end(ap);
   return code;
}
// ------------------------------------------------------------------ tiny host 3x3 helpers (double)
struct M3d
{
   double m[9];
};
M3d m3_identity() { return M3d{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
M3d m3_mul(const M3d &a, const M3d &b)
{
   M3d o;
   for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
         o.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
   return o;
}
M3d m3_T(const M3d &a) { return M3d{{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}}; }
void m3_mulv(const M3d &a, const double v[3], double o[3])
{
   double x = a.m[0] * v[0] + a.m[1] * v[1] + a.m[2] * v[2];
   double y = a.m[3] * v[0] + a.m[4] * v[1] + a.m[5] * v[2];
   double z = a.m[6] * v[0] + a.m[7] * v[1] + a.m[8] * v[2];
   o[0] = x, o[1] = y, o[2] = z;
}
// rotation Q with Q * ez = k (k unit): columns (x', y', k) of a right-handed orthonormal basis
M3d frame_with_z(const double k[3])
{
   int least = std::fabs(k[0]) <= std::fabs(k[1]) ? (std::fabs(k[0]) <= std::fabs(k[2]) ? 0 : 2) : (std::fabs(k[1]) <= std::fabs(k[2]) ? 1 : 2);
   double h[3] = {0, 0, 0};
   h[least] = 1.0;
   double d = h[0] * k[0] + h[1] * k[1] + h[2] * k[2];
   double x[3] = {h[0] - d * k[0], h[1] - d * k[1], h[2] - d * k[2]};
   double n = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
   x[0] /= n, x[1] /= n, x[2] /= n;
   double y[3] = {k[1] * x[2] - k[2] * x[1], k[2] * x[0] - k[0] * x[2], k[0] * x[1] - k[1] * x[0]};
   return M3d{{x[0], y[0], k[0], x[1], y[1], k[1], x[2], y[2], k[2]}};
}
int joint_ndof(int t) { return mh::dof_count(t); }
int joint_ncfg(int t) { return mh::cfg_count(t); }
// Host-only part of model creation: validation and the engine's joint order (depth-first, parents first).
struct Plan
{
   std::vector<int> order;     // engine index -> caller index
   std::vector<int> engine_of; // caller index -> engine index
   std::vector<int> dofo, cfgo; // per caller joint: offsets into the concatenated index maps
   std::vector<std::vector<int>> children; // by caller index
   std::vector<int> eparent, etype;        // engine order
   std::string key;
};

mh_status plan_model(const mh_model_desc *d, Plan &P)
{
   if (!d)
      return fail(MH_ERR_INVALID_ARGUMENT, "desc is NULL");
   const int n = d->n_joints;
   if (n <= 0)
      return fail(MH_ERR_INVALID_ARGUMENT, "n_joints = %d", n);
   if (!d->parent || !d->joint_type || !d->axis || !d->X_before || !d->X_com || !d->inertia_J || !d->inertia_mass || !d->inertia_com
       || !d->dof_indices || !d->cfg_indices)
      return fail(MH_ERR_INVALID_ARGUMENT, "a model array is NULL");
   if (d->nq < 0 || d->nv < 0)
      return fail(MH_ERR_BAD_DIMENSION, "nq = %d, nv = %d", d->nq, d->nv);
   P.dofo.assign(n + 1, 0), P.cfgo.assign(n + 1, 0);
   for (int i = 0; i < n; i++)
   {
      const int t = d->joint_type[i];
      if (t < MH_JOINT_REVOLUTE || t > MH_JOINT_SPHERICAL)
         return fail(MH_ERR_UNSUPPORTED_JOINT, "joint %d has unsupported kind %d", i, t);
      if (d->parent[i] < -1 || d->parent[i] >= n || d->parent[i] == i)
         return fail(MH_ERR_BAD_TOPOLOGY, "joint %d has parent %d", i, d->parent[i]);
      P.dofo[i + 1] = P.dofo[i] + joint_ndof(t);
      P.cfgo[i + 1] = P.cfgo[i] + joint_ncfg(t);
   }
   {
      std::vector<char> seen_v(d->nv, 0), seen_q(d->nq, 0);
      for (int k = 0; k < P.dofo[n]; k++)
      {
         const int r = d->dof_indices[k];
         if (r < 0 || r >= d->nv || seen_v[r])
            return fail(MH_ERR_BAD_TOPOLOGY, "dof_indices[%d] = %d is out of range or repeated (nv = %d)", k, r, d->nv);
         seen_v[r] = 1;
      }
      for (int k = 0; k < P.cfgo[n]; k++)
      {
         const int r = d->cfg_indices[k];
         if (r < 0 || r >= d->nq || seen_q[r])
            return fail(MH_ERR_BAD_TOPOLOGY, "cfg_indices[%d] = %d is out of range or repeated (nq = %d)", k, r, d->nq);
         seen_q[r] = 1;
      }
   }
   // engine order: depth-first pre-order, children in the caller's order (chains stay contiguous)
   P.children.assign(n, {});
   std::vector<int> roots;
   for (int i = 0; i < n; i++)
      (d->parent[i] < 0 ? roots : P.children[d->parent[i]]).push_back(i);
   P.order.clear();
   P.order.reserve(n);
   {
      std::vector<int> stack(roots.rbegin(), roots.rend());
      while (!stack.empty())
      {
         int i = stack.back();
         stack.pop_back();
         P.order.push_back(i);
         for (auto it = P.children[i].rbegin(); it != P.children[i].rend(); ++it)
            stack.push_back(*it);
      }
   }
   if ((int)P.order.size() != n)
      return fail(MH_ERR_LOOP_CLOSURE, "parent[] contains a cycle: %d of %d joints are reachable from the root", (int)P.order.size(), n);
   P.engine_of.assign(n, 0);
   for (int e = 0; e < n; e++)
      P.engine_of[P.order[e]] = e;
   P.eparent.assign(n, -1), P.etype.assign(n, 0);
   unsigned long long h = 1469598103934665603ull; // FNV-1a over (n, parents, kinds) in engine order
   auto mix = [&](int v) {
      for (int b = 0; b < 4; b++)
      {
         h ^= (unsigned long long)((v >> (8 * b)) & 0xff);
         h *= 1099511628211ull;
      }
   };
   mix(n);
   for (int e = 0; e < n; e++)
   {
      const int i = P.order[e];
      P.eparent[e] = d->parent[i] < 0 ? -1 : P.engine_of[d->parent[i]];
      P.etype[e] = d->joint_type[i];
      mix(P.eparent[e]);
      mix(P.etype[e]);
   }
   char buf[32];
   snprintf(buf, sizeof buf, "%016llx", h);
   P.key = buf;
   return MH_OK;
}

// Everything mh_model_create derives from the description, and nothing else.  Immutable once compiled, with one exception:
// mh_model_set_joint_source_modes sets the MF_LOCKED bits in `meta` and uploads the records again.
struct ModelTables
{
   int n = 0, nq = 0, nv = 0, n_slots = 0;
   std::vector<int> meta, dof_map, cfg_map;
   std::vector<double> consts;
   std::vector<int> engine_of; // caller joint index -> engine index
   std::vector<int> prog;     // event program of the depth-first kernels
   std::vector<int> prog_seq; // the same walk with the siblings in engine order (the kernels that read AoS rows through LDS windows)
   int rnea_stack = 0, aba_stack = 0, aba_hand = 0; // per-lane slots: depth stacks, ABA hand-over
   int pair_stack = 0;                              // ... of the fused RNEA + ABA walk (aba_dfs_kernel<.., PAIR>)
   double nonleaf_fraction = 1.0;                   // share of bodies with children: those are the ones that touch the depth stack
   int n_nonadjacent = 0; // bodies whose parent is not the body before them in engine order (branch points of the tree)
   // mh_gravity_gradient_*: subtree masses (engine order) and, per body, the matrix columns of unrelated joints (mh_gravity_kernels.h)
   std::vector<double> sub_mass;
   std::vector<int> grav_zero_ofs, grav_zero_cols;
   // mh_apparent_inertia_inverse_*: Euler tour of the tree and the slots of the six-column accelerations (mh_response_kernels.h), and
   // the workspace slots per lane of that kernel: the model's, 36 per body with a child that does not directly follow it, 6 per DoF
   std::vector<int> resp_info;
   int resp_slots = 0, resp_a_base = 0, resp_u_base = 0;
   // mh_mass_matrix_inverse_*: per DoF index of the model's index map, 8 * engine index of the joint that owns it + its place among the
   // joint's DoFs (-1: no joint); the kernel (mh_minv_kernels.h) works in the workspace slots of the apparent-inertia kernel
   std::vector<int> minv_owner;
   // mh_rnea_derivatives_* / mh_aba_derivatives_*: first workspace slot of every body in that kernel's own plan (mh_rnea_deriv_kernels.h)
   // and its slots per lane
   std::vector<int> deriv_slot;
   int deriv_slots = 0;
   // mh_model_inertial_parameters / mh_rnea_parameters_* / mh_aba_parameters_*: the description's ten inertial numbers per joint, in
   // mh_model_desc order (host only: the kernels of mh_params_kernels.h take them per configuration from the call)
   std::vector<double> inertial_parameters;
   int ident_maps = 0; // the engine-order index maps are the identity
   int dense_maps = 0; // nq / nv equal the joints' totals (no unused matrix rows): rows can be staged as dense blocks
   // an output of nv columns may be q itself: nq == nv, every joint with DoFs is revolute, and its row of q is its row of qd.  A kernel
   // reads a revolute joint's angle once (cos, sin live on in registers or workspace) and writes only that joint's entry of the output;
   // prismatic and planar coordinates are read from q again after the joint's output has been stored (joint_again, mh_kernels.h)
   int q_may_be_out = 0;
   uint32_t warnings = 0;    // MH_WARN_* bits set by mh_model_create (mh_model_warnings)
   std::string warning_text; // ... and what they mean for this model
   std::string topo_key;
};

// ---- the tree in engine order: children lists (ascending, which is the caller's order among siblings) and one depth-first walk for
// everything that needs one.  The stack is explicit: a chain of 100 000 bodies is a model too.
struct EngineTree
{
   std::vector<std::vector<int>> kids;
   std::vector<int> roots;
};
EngineTree engine_tree(const Plan &P)
{
   EngineTree t;
   t.kids.resize(P.eparent.size());
   for (int e = 0; e < (int)P.eparent.size(); e++)
      (P.eparent[e] >= 0 ? t.kids[P.eparent[e]] : t.roots).push_back(e);
   return t;
}
// visit(e) on the way down, pop(e) once every child of e has been popped
template <class Visit, class Pop>
void walk_depth_first(const EngineTree &t, Visit visit, Pop pop)
{
   std::vector<std::pair<int, size_t>> path; // (body, next child to walk)
   for (int r : t.roots)
   {
      visit(r);
      path.emplace_back(r, 0);
      while (!path.empty())
      {
         const int e = path.back().first;
         if (path.back().second < t.kids[e].size())
         {
            const int c = t.kids[e][path.back().second++];
            visit(c);
            path.emplace_back(c, 0);
         }
         else
         {
            pop(e);
            path.pop_back();
         }
      }
   }
}

// ---- canonical frames: Q_e maps the canonical after-joint axes of joint e to Mecano's after-joint axes, O_e is the canonical origin in
// Mecano's after-joint frame (engine order)
struct CanonicalFrames
{
   std::vector<M3d> Q;
   std::vector<std::array<double, 3>> O;
   std::vector<char> aligned; // the joint's origin lies on its parent's canonical x axis
};
mh_status canonical_frames(const mh_model_desc *d, const Plan &P, CanonicalFrames &F)
{
   const int n = d->n_joints;
   const std::vector<int> &order = P.order;
   std::vector<M3d> &Q = F.Q;
   Q.resize(n);
   for (int e = 0; e < n; e++)
   {
      const int i = order[e];
      const int t = d->joint_type[i];
      if (t == MH_JOINT_REVOLUTE || t == MH_JOINT_PRISMATIC)
      {
         const double *a = d->axis + 3 * i;
         const double nrm = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
         if (!(std::fabs(nrm - 1.0) <= 1.0e-6))
            return fail(MH_ERR_BAD_AXIS, "joint %d: axis (%g, %g, %g) is not a unit vector", i, a[0], a[1], a[2]);
         const double k[3] = {a[0] / nrm, a[1] / nrm, a[2] / nrm};
         Q[e] = frame_with_z(k);
      }
      else
         Q[e] = m3_identity();
   }

   // The frame after a 1-DoF joint may still turn about and slide along its own axis (both commute with the joint's motion).  That freedom
   // is spent on the joint's FIRST child (engine order: the next joint): origin and x axis are chosen so that the child's origin lies on the
   // x axis, p_b(child) = (a, 0, 0) -- two of the three translation components of that child's pose are structural zeros, which the
   // specialised kernels fold at compile time (Tree<TP>::p_aligned; the run-time-topology kernels just multiply by 0.0).  O[e] = origin of
   // the canonical frame of joint e in Mecano's after-joint frame (on the axis); children first, because a child's own slide moves its origin.
   std::vector<std::array<double, 3>> &O = F.O;
   O.assign(n, std::array<double, 3>{0.0, 0.0, 0.0});
   F.aligned.assign(n, 0);
   for (int e = n - 2; e >= 0; e--)
   {
      const int i = order[e], t = d->joint_type[i], ic = order[e + 1];
      if ((t != MH_JOINT_REVOLUTE && t != MH_JOINT_PRISMATIC) || d->parent[ic] != i)
         continue;
      M3d Rbc;
      std::memcpy(Rbc.m, d->X_before + 12 * ic, sizeof Rbc.m);
      double w0[3], w[3];
      m3_mulv(Rbc, O[e + 1].data(), w0);
      for (int k = 0; k < 3; k++)
         w0[k] += d->X_before[12 * ic + 9 + k];
      m3_mulv(m3_T(Q[e]), w0, w);
      const double delta = w[2], rho = std::hypot(w[0], w[1]);
      const double cphi = rho > 1.0e-12 ? w[0] / rho : 1.0, sphi = rho > 1.0e-12 ? w[1] / rho : 0.0;
      const double slide[3] = {0.0, 0.0, delta};
      m3_mulv(Q[e], slide, O[e].data());
      M3d Rz = m3_identity();
      Rz.m[0] = cphi, Rz.m[1] = -sphi, Rz.m[3] = sphi, Rz.m[4] = cphi;
      Q[e] = m3_mul(Q[e], Rz);
      F.aligned[e + 1] = 1;
   }
   return MH_OK;
}

// ---- the two places where this engine consciously departs from the reference: told to the caller, not hidden
void divergence_warnings(const mh_model_desc *d, const Plan &P, ModelTables *m)
{
   const int n = d->n_joints;
   char buf[512];
   // (1) tools/MecanoFactories.java:51, 237-248: a revolute axis that geometricallyEquals X, Y or Z within 1e-7 WITHOUT being that axis
   // gets a joint rotation about the exact coordinate axis while the unit twist keeps the axis as given; the engine uses the given axis for both
   for (int i = 0; i < n; i++)
   {
      if (d->joint_type[i] != MH_JOINT_REVOLUTE)
         continue;
      const double *a = d->axis + 3 * i;
      for (int k = 0; k < 3; k++)
      {
         const double dx = a[0] - (k == 0), dy = a[1] - (k == 1), dz = a[2] - (k == 2);
         const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
         if (dist <= 1.0e-7 && dist > 0.0)
         {
            if (!(m->warnings & MH_WARN_NEAR_COORDINATE_AXIS))
            {
               snprintf(buf, sizeof buf,
                        "joint %d: axis (%.17g, %.17g, %.17g) is within 1e-7 of the %c axis but not on it: Mecano rotates such a joint about the exact "
                        "coordinate axis and keeps the given axis in its unit twist (MecanoFactories.java:237-248); this engine uses the given axis for "
                        "both, results differ from Mecano's by up to ~4e-7 relative. ",
                        i, a[0], a[1], a[2], "XYZ"[k]);
               m->warning_text += buf;
            }
            m->warnings |= MH_WARN_NEAR_COORDINATE_AXIS;
            break;
         }
      }
   }
   // (2) spatial/interfaces/FixedFrameSpatialInertiaBasics.java:167-176: SpatialInertia.add skips the renormalisation of the centre of
   // mass when the summed mass is under 1e-7; the mass matrix of a body whose composite with a child's subtree stays under it differs
   std::vector<double> sub(n, 0.0);
   for (int e = n - 1; e >= 0; e--)
   {
      const int i = P.order[e];
      sub[i] += d->inertia_mass[i];
      if (d->parent[i] >= 0)
         sub[d->parent[i]] += sub[i];
   }
   for (int i = 0; i < n; i++)
      for (int ch : P.children[i])
         if (std::fabs(d->inertia_mass[i] + sub[ch]) < 1.0e-7)
         {
            if (!(m->warnings & MH_WARN_TINY_COMPOSITE_MASS))
            {
               snprintf(buf, sizeof buf,
                        "joint %d: the body's mass plus the subtree of joint %d is %.3g < 1e-7: Mecano's SpatialInertia.add leaves such a composite's "
                        "centre of mass un-normalised (FixedFrameSpatialInertiaBasics.java:174-175); this engine's mass matrix stays consistent "
                        "with its inverse dynamics and differs from Mecano's by less than the masses involved (<= 1e-6). ",
                        i, ch, d->inertia_mass[i] + sub[ch]);
               m->warning_text += buf;
            }
            m->warnings |= MH_WARN_TINY_COMPOSITE_MASS;
         }
}

// ---- index maps re-concatenated in ENGINE order: the offset of a joint in them is then a function of the topology alone
struct EngineOffsets
{
   std::vector<int> dof, cfg; // [n + 1]: where a joint's entries start in dof_map / cfg_map
};
EngineOffsets index_maps(const mh_model_desc *d, const Plan &P, ModelTables *m)
{
   const int n = d->n_joints;
   const std::vector<int> &dofo = P.dofo, &cfgo = P.cfgo;
   EngineOffsets ofs;
   std::vector<int> &edofo = ofs.dof, &ecfgo = ofs.cfg;
   edofo.assign(n + 1, 0), ecfgo.assign(n + 1, 0);
   for (int e = 0; e < n; e++)
   {
      const int i = P.order[e];
      edofo[e + 1] = edofo[e] + (dofo[i + 1] - dofo[i]);
      ecfgo[e + 1] = ecfgo[e] + (cfgo[i + 1] - cfgo[i]);
      for (int k = dofo[i]; k < dofo[i + 1]; k++)
         m->dof_map.push_back(d->dof_indices[k]);
      for (int k = cfgo[i]; k < cfgo[i + 1]; k++)
         m->cfg_map.push_back(d->cfg_indices[k]);
   }
   m->dense_maps = (edofo[n] == d->nv && ecfgo[n] == d->nq);
   m->ident_maps = m->dense_maps;
   for (int k = 0; m->ident_maps && k < edofo[n]; k++)
      m->ident_maps = m->dof_map[k] == k;
   for (int k = 0; m->ident_maps && k < ecfgo[n]; k++)
      m->ident_maps = m->cfg_map[k] == k;
   m->q_may_be_out = d->nq == d->nv;
   for (int i = 0; m->q_may_be_out && i < n; i++)
      if (dofo[i + 1] > dofo[i])
         m->q_may_be_out = d->joint_type[i] == MH_JOINT_REVOLUTE && d->cfg_indices[cfgo[i]] == d->dof_indices[dofo[i]];
   if (m->dof_map.empty())
      m->dof_map.push_back(0);
   if (m->cfg_map.empty())
      m->cfg_map.push_back(0);
   return ofs;
}

// ---- body records: flags, the workspace slot plan of the sweep kernels, the constants in the canonical frames
void body_records(const mh_model_desc *d, const Plan &P, const CanonicalFrames &F, const EngineOffsets &ofs, ModelTables *m)
{
   const int n = d->n_joints;
   const std::vector<int> &engine_of = P.engine_of;
   const std::vector<std::vector<int>> &children = P.children;
   const std::vector<M3d> &Q = F.Q;
   const std::vector<std::array<double, 3>> &O = F.O;
   m->meta.assign((size_t)n * mh::MI_STRIDE, 0);
   m->consts.assign((size_t)n * mh::MC_STRIDE, 0.0);
   int slots = 0;
   for (int e = 0; e < n; e++)
   {
      const int i = P.order[e];
      const int t = d->joint_type[i];
      const int pe = d->parent[i] < 0 ? -1 : engine_of[d->parent[i]];
      int *mi = &m->meta[(size_t)e * mh::MI_STRIDE];
      double *c = &m->consts[(size_t)e * mh::MC_STRIDE];
      mi[mh::MI_PARENT] = pe;
      mi[mh::MI_TYPE] = t;
      mi[mh::MI_DOF] = ofs.dof[e];
      mi[mh::MI_CFG] = ofs.cfg[e];
      mi[mh::MI_EXT] = i;
      int flags = 0;
      if (pe >= 0 && pe == e - 1)
         flags |= mh::MF_PARENT_ADJ;
      else if (pe >= 0)
         m->n_nonadjacent++;
      bool nonadj_child = false;
      for (int ch : children[i])
         if (engine_of[ch] != e + 1)
            nonadj_child = true;
      if (nonadj_child)
         flags |= mh::MF_STORE_VA | mh::MF_HAS_ACC;
      if (pe >= 0 && pe != e - 1)
      {
         // first contributor = highest engine index among the non-adjacent children of the parent
         int hi = -1;
         for (int ch : children[d->parent[i]])
            if (engine_of[ch] != pe + 1)
               hi = std::max(hi, engine_of[ch]);
         if (hi == e)
            flags |= mh::MF_ACC_FIRST;
      }
      mi[mh::MI_FLAGS] = flags;
      mi[mh::MI_SLOT_JP] = slots, slots += (t == MH_JOINT_REVOLUTE ? 2 : 0);
      mi[mh::MI_SLOT_F] = slots, slots += 8;
      mi[mh::MI_SLOT_C] = slots, slots += 6;
      mi[mh::MI_SLOT_VA] = slots, slots += (nonadj_child ? 12 : 0);
      mi[mh::MI_SLOT_IA] = slots, slots += (nonadj_child ? 40 : 0); // ABA: 21 | CRBA: 10 | Coriolis: 10 + 30
      mi[mh::MI_SLOT_LK] = slots, slots += (mh::dof_count(t) >= 3 ? 27 : 0); // multi-DoF joints: U, D^-1, u | locked: IA, pA

      // X_before' = Qp^T X_before Q : canonical before-joint frame in the parent's canonical after-joint frame
      const M3d Qp = pe < 0 ? m3_identity() : Q[pe];
      M3d Rb;
      std::memcpy(Rb.m, d->X_before + 12 * i, sizeof Rb.m);
      const M3d Rb2 = m3_mul(m3_mul(m3_T(Qp), Rb), Q[e]);
      double pb2[3], pb0[3];
      m3_mulv(Rb, O[e].data(), pb0); // the canonical origin of this joint, then relative to the parent's canonical origin
      for (int k = 0; k < 3; k++)
         pb0[k] += d->X_before[12 * i + 9 + k] - (pe < 0 ? 0.0 : O[pe][k]);
      m3_mulv(m3_T(Qp), pb0, pb2);
      if (F.aligned[e])
         pb2[1] = 0.0, pb2[2] = 0.0; // (a, 0, 0) by construction: what is left is rounding
      for (int k = 0; k < 9; k++)
         c[mh::MC_RB + k] = Rb2.m[k];
      for (int k = 0; k < 3; k++)
         c[mh::MC_PB + k] = pb2[k];
      // body-fixed -> canonical after-joint: R' = Q^T Rc, p' = Q^T pc
      M3d Rc;
      std::memcpy(Rc.m, d->X_com + 12 * i, sizeof Rc.m);
      const M3d Rf = m3_mul(m3_T(Q[e]), Rc);
      double pf[3], pf0[3];
      for (int k = 0; k < 3; k++)
         pf0[k] = d->X_com[12 * i + 9 + k] - O[e][k];
      m3_mulv(m3_T(Q[e]), pf0, pf);
      for (int k = 0; k < 9; k++)
         c[mh::MC_RF + k] = Rf.m[k];
      for (int k = 0; k < 3; k++)
         c[mh::MC_PF + k] = pf[k];
      // canonical after-joint -> Mecano's after-joint frame: x = Q x' + O (joint wrench outputs)
      for (int k = 0; k < 9; k++)
         c[mh::MC_QA + k] = Q[e].m[k];
      for (int k = 0; k < 3; k++)
         c[mh::MC_OA + k] = O[e][k];
      // spatial inertia about the canonical after-joint origin.  J is the rotational inertia about the ORIGIN of the
      // body-fixed frame with the CoM at c_b there (spatial/interfaces/SpatialInertiaReadOnly.java:394-415).
      const double mass = d->inertia_mass[i];
      const double *cb = d->inertia_com + 3 * i;
      M3d J;
      std::memcpy(J.m, d->inertia_J + 9 * i, sizeof J.m);
      const M3d Jr = m3_mul(m3_mul(Rf, J), m3_T(Rf)); // about the body-fixed origin, canonical axes
      double cr[3];
      m3_mulv(Rf, cb, cr); // CoM relative to the body-fixed origin, canonical axes
      // shift the origin from the body-fixed origin (at pf) to the after-joint origin: c' = cr + pf
      const double h0[3] = {mass * cr[0], mass * cr[1], mass * cr[2]};
      const double dd = 2.0 * (pf[0] * h0[0] + pf[1] * h0[1] + pf[2] * h0[2]) + mass * (pf[0] * pf[0] + pf[1] * pf[1] + pf[2] * pf[2]);
      double I[9];
      for (int r = 0; r < 3; r++)
         for (int s = 0; s < 3; s++)
            I[3 * r + s] = Jr.m[3 * r + s] + (r == s ? dd : 0.0) - (pf[r] * h0[s] + h0[r] * pf[s] + mass * pf[r] * pf[s]);
      c[mh::MC_M] = mass;
      for (int k = 0; k < 3; k++)
         c[mh::MC_H + k] = h0[k] + mass * pf[k];
      // (mh_params_kernels.h, inertia_from_parameters: the same map on the device, per configuration)
      c[mh::MC_I + 0] = I[0], c[mh::MC_I + 1] = 0.5 * (I[1] + I[3]), c[mh::MC_I + 2] = 0.5 * (I[2] + I[6]);
      c[mh::MC_I + 3] = I[4], c[mh::MC_I + 4] = 0.5 * (I[5] + I[7]), c[mh::MC_I + 5] = I[8];
   }
   m->n_slots = std::max(slots, 1);
}

void inertial_parameters(const mh_model_desc *d, ModelTables *m)
{
   const int n = d->n_joints;
   m->inertial_parameters.resize((size_t)n * mh::PARAMS_PER_BODY);
   for (int i = 0; i < n; i++)
   {
      double *p = &m->inertial_parameters[(size_t)i * mh::PARAMS_PER_BODY];
      const double *J = d->inertia_J + 9 * i;
      p[0] = d->inertia_mass[i];
      for (int k = 0; k < 3; k++)
         p[1 + k] = d->inertia_com[3 * i + k];
      p[4] = J[0], p[5] = 0.5 * (J[1] + J[3]), p[6] = 0.5 * (J[2] + J[6]), p[7] = J[4], p[8] = 0.5 * (J[5] + J[7]), p[9] = J[8];
   }
}

// ---- gravity gradient (mh_gravity_kernels.h): the subtree masses do not depend on q; the zero pattern of its matrix is the topology's
void gravity_tables(const mh_model_desc *d, const Plan &P, const EngineOffsets &ofs, ModelTables *m)
{
   const int n = d->n_joints;
   const std::vector<int> &edofo = ofs.dof;
   m->sub_mass.assign(n, 0.0);
   for (int e = n - 1; e >= 0; e--)
   {
      m->sub_mass[e] += m->consts[(size_t)e * mh::MC_STRIDE + mh::MC_M];
      if (P.eparent[e] >= 0)
         m->sub_mass[P.eparent[e]] += m->sub_mass[e];
   }
   std::vector<char> owned(d->nv, 0);
   for (int k = 0; k < edofo[n]; k++)
      owned[m->dof_map[k]] = 1;
   std::vector<char> related((size_t)n * n, 0); // related[a * n + b]: a == b or one is an ancestor of the other
   for (int e = 0; e < n; e++)
      for (int a = e; a >= 0; a = P.eparent[a])
         related[(size_t)e * n + a] = related[(size_t)a * n + e] = 1;
   m->grav_zero_ofs.assign(n + 2, 0);
   for (int e = 0; e < n; e++)
   {
      if (edofo[e + 1] > edofo[e]) // (a joint without DoFs has no rows)
      {
         for (int b = 0; b < n; b++)
            if (!related[(size_t)e * n + b])
               for (int k = edofo[b]; k < edofo[b + 1]; k++)
                  m->grav_zero_cols.push_back(m->dof_map[k]);
         for (int r = 0; r < d->nv; r++)
            if (!owned[r])
               m->grav_zero_cols.push_back(r);
      }
      m->grav_zero_ofs[e + 1] = (int)m->grav_zero_cols.size();
   }
   for (int r = 0; r < d->nv; r++)
      if (!owned[r])
         m->grav_zero_cols.push_back(r);
   m->grav_zero_ofs[n + 1] = (int)m->grav_zero_cols.size();
   if (m->grav_zero_cols.empty())
      m->grav_zero_cols.push_back(0);
}

// ---- apparent inertia inverses (mh_response_kernels.h): which body lies under which is the topology's
void response_tables(const EngineTree &tree, const EngineOffsets &ofs, ModelTables *m)
{
   const int n = m->n;
   m->resp_info.assign((size_t)n * mh::RI_STRIDE, 0);
   int clock = 0, n_a = 0;
   walk_depth_first(
      tree, [&](int e) { m->resp_info[(size_t)e * mh::RI_STRIDE + mh::RI_TIN] = clock++; },
      [&](int e) { m->resp_info[(size_t)e * mh::RI_STRIDE + mh::RI_TOUT] = clock++; });
   for (int e = 0; e < n; e++)
      m->resp_info[(size_t)e * mh::RI_STRIDE + mh::RI_SLOT_A] = (m->meta[(size_t)e * mh::MI_STRIDE + mh::MI_FLAGS] & mh::MF_STORE_VA) ? 36 * n_a++ : -1;
   m->resp_a_base = m->n_slots;
   m->resp_u_base = m->resp_a_base + 36 * n_a;
   m->resp_slots = m->resp_u_base + 6 * ofs.dof[n];
}

// ---- inverse of the joint-space inertia matrix (mh_minv_kernels.h): which joint owns which DoF index
void dof_owners(const EngineOffsets &ofs, ModelTables *m)
{
   m->minv_owner.assign((size_t)std::max(1, m->nv), -1);
   for (int e = 0; e < m->n; e++)
      for (int k = ofs.dof[e]; k < ofs.dof[e + 1]; k++)
         m->minv_owner[m->dof_map[k]] = 8 * e + (k - ofs.dof[e]);
}

// ---- derivatives of the inverse dynamics (mh_rnea_deriv_kernels.h): that kernel's own slot plan
void derivative_slot_plan(ModelTables *m)
{
   const int n = m->n;
   m->deriv_slot.assign((size_t)std::max(1, n), 0);
   m->deriv_slots = 0;
   for (int e = 0; e < n; e++)
   {
      m->deriv_slot[e] = m->deriv_slots;
      m->deriv_slots += (m->meta[(size_t)e * mh::MI_STRIDE + mh::MI_FLAGS] & mh::MF_STORE_VA) ? mh::DS_BRANCH : mh::DS_BODY;
   }
   m->deriv_slots = std::max(m->deriv_slots, 1);
}

// ---- depth-first kernels: children counts, stack-frame / hand-over offsets, event program (mh_dfs_kernels.h)
// The walk: depth-first, the children of a body in the order [those with children of their own | the leaves].  A child's contribution
// to its parent (wrench; articulated inertia + bias wrench) is either accumulated in the parent's frame (read-modify-write of 6 / 27 /
// 33 slots) or handed over in registers, the carry.  The carry survives a LEAF sibling's two events (they never touch it), so the
// last child with children of its own sets it and every leaf behind it adds to it: only the other children with subtrees go through
// the frame (128-body tree of configs[4]: 26 of 127 child pops, before the leaves were sorted behind: 64).
// (The kernels that read AoS rows through LDS windows consume the matrices in engine order and refill synchronously on a jump: they
// keep a program in engine order -- prog_seq --, with the same carry rule applied to whatever leaves happen to come last.)
void event_program(const Plan &P, EngineTree tree, const std::vector<int> &nch, bool leaves_last, std::vector<int> &prog)
{
   const int n = (int)nch.size();
   std::vector<std::vector<int>> &kids = tree.kids;
   if (leaves_last)
      for (int e = 0; e < n; e++)
         std::stable_partition(kids[e].begin(), kids[e].end(), [&](int c) { return nch[c] > 0; });
   std::vector<size_t> pop_at(n, 0);
   auto visit = [&](int e) {
      int ev = e << mh::EV_BODY_SHIFT;
      if (!prog.empty() && P.eparent[e] >= 0 && !(prog.back() & mh::EV_POP) && (prog.back() >> mh::EV_BODY_SHIFT) == P.eparent[e])
         ev |= mh::EV_PARENT_REGS;
      prog.push_back(ev);
   };
   auto pop = [&](int e) {
      int pv = (e << mh::EV_BODY_SHIFT) | mh::EV_POP;
      if (prog.back() == (e << mh::EV_BODY_SHIFT) + (prog.back() & mh::EV_PARENT_REGS))
         pv |= mh::EV_LEAF; // the previous event is VISIT(e)
      pop_at[e] = prog.size();
      prog.push_back(pv);
   };
   walk_depth_first(tree, visit, pop);
   for (int e = 0; e < n; e++)
   {
      const std::vector<int> &k = kids[e];
      if (k.empty())
         continue;
      int first_carried = 0; // the last child with children of its own (only leaves behind it), or the first child
      for (size_t i = 0; i < k.size(); i++)
         if (nch[k[i]] > 0)
            first_carried = (int)i;
      for (size_t i = 0; i < k.size(); i++)
      {
         int &ev = prog[pop_at[k[i]]];
         if ((int)i < first_carried)
            ev |= i == 0 ? mh::EV_ACC_FIRST : 0;
         else
            ev |= (int)i == first_carried ? mh::EV_LAST_CHILD : mh::EV_CARRY_ADD;
      }
      if (first_carried > 0)
         prog[pop_at[e]] |= mh::EV_ACC_USED;
   }
}
void depth_first_tables(const Plan &P, const EngineTree &tree, ModelTables *m)
{
   const int n = m->n;
   std::vector<int> nch(n, 0), ofs_r(n, 0), ofs_a(n, 0), ofs_p(n, 0);
   for (int e = 0; e < n; e++)
      if (P.eparent[e] >= 0)
         nch[P.eparent[e]]++;
   int hand = 0;
   for (int e = 0; e < n; e++)
   {
      const int pe = P.eparent[e], t = P.etype[e];
      ofs_r[e] = pe < 0 ? 0 : ofs_r[pe] + mh::rnea_frame_slots(P.etype[pe], nch[pe]);
      ofs_a[e] = pe < 0 ? 0 : ofs_a[pe] + mh::aba_frame_slots(P.etype[pe], nch[pe]);
      m->rnea_stack = std::max(m->rnea_stack, ofs_r[e] + mh::rnea_frame_slots(t, nch[e]));
      m->aba_stack = std::max(m->aba_stack, ofs_a[e] + mh::aba_frame_slots(t, nch[e]));
      ofs_p[e] = pe < 0 ? 0 : ofs_p[pe] + mh::pair_frame_slots(P.etype[pe], nch[pe]);
      m->pair_stack = std::max(m->pair_stack, ofs_p[e] + mh::pair_frame_slots(t, nch[e]));
      int *mi = &m->meta[(size_t)e * mh::MI_STRIDE];
      mi[mh::MI_NCH] = nch[e], mi[mh::MI_DFS_R] = ofs_r[e], mi[mh::MI_DFS_A] = ofs_a[e], mi[mh::MI_HAND] = hand;
      hand += mh::aba_hand_slots(t, nch[e]);
      if (pe >= 0)
      {
         const int pj = mh::jx_slots(P.etype[pe]);
         mi[mh::MI_PFR_R] = ofs_r[pe], mi[mh::MI_PVA_R] = ofs_r[pe] + 6 + pj;
         mi[mh::MI_PFR_A] = ofs_a[pe], mi[mh::MI_PV_A] = ofs_a[pe] + 12 + pj, mi[mh::MI_PACC_A] = ofs_a[pe] + 18 + pj;
      }
      if (t == MH_JOINT_REVOLUTE || t == MH_JOINT_PRISMATIC)
         mi[mh::MI_ROW_Q] = m->cfg_map[mi[mh::MI_CFG]], mi[mh::MI_ROW_V] = m->dof_map[mi[mh::MI_DOF]];
   }
   m->aba_hand = std::max(hand, 1);
   m->nonleaf_fraction = (double)std::count_if(nch.begin(), nch.end(), [](int c) { return c > 0; }) / (double)n;
   m->rnea_stack = std::max(m->rnea_stack, 1), m->aba_stack = std::max(m->aba_stack, 6);
   event_program(P, tree, nch, true, m->prog);
   event_program(P, tree, nch, false, m->prog_seq);
}

// The description -> its tables.  `m` is left as it was when the description is refused (MH_ERR_BAD_AXIS: the one check plan_model leaves).
mh_status compile_model(const mh_model_desc *d, const Plan &P, ModelTables &T)
{
   ModelTables *m = &T;
   CanonicalFrames F;
   mh_status st = canonical_frames(d, P, F);
   if (st != MH_OK)
      return st;
   m->n = d->n_joints, m->nq = d->nq, m->nv = d->nv;
   m->engine_of = P.engine_of;
   m->topo_key = P.key;
   divergence_warnings(d, P, m);
   const EngineOffsets ofs = index_maps(d, P, m);
   body_records(d, P, F, ofs, m);
   inertial_parameters(d, m);
   gravity_tables(d, P, ofs, m);
   const EngineTree tree = engine_tree(P);
   response_tables(tree, ofs, m);
   dof_owners(ofs, m);
   derivative_slot_plan(m);
   depth_first_tables(P, tree, m);
   return MH_OK;
}
} // namespace
