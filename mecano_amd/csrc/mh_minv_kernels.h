// mh_minv_kernels.h -- columns of the inverse of the joint-space inertia matrix, H^-1 e_c (run-time topology, one lane per configuration,
// gfx950).
//
// Column c is the change of the joint accelerations when a unit effort acts on DoF c: MultiBodyResponseCalculator's applyJointWrench
// (algorithms/MultiBodyResponseCalculator.java:685-735) with the recursion behind it (:1206-1252 climb, :1301-1338 descent), which is
// what computeJointApparentInertiaInverse (:512-590) evaluates per DoF of a joint.  The articulated-body recursion of
// mh_response_kernels.h does the work; H is not formed and nothing dense is factorised:
//   1. minv_articulated_inertias (phase 1 of apparent_inertia_kernel): IA, U and D^-1 of every joint; an ACCELERATION_SOURCE joint
//      hands IA up undiminished and gets D^-1 = 0, so that its rows and columns come out as zeros without a branch.
//   2. per column c, DoF l of joint j: u+_j = e_l, pa+ = U D^-1 u+ handed to the parent, then u+ = -S^T pA+, pa+ = pA+ + U D^-1 u+
//      up the path to the root; u+ of every joint of the path is kept (6 slots per DoF: one per column of the group).
//   3. over ALL bodies, root outwards: qdd+ = D^-1 (u+ - U^T a+_parent) with u+ = 0 off the column's path, a+ = X a+_parent + S qdd+;
//      qdd+ is the column's entry in the rows of that body's DoFs.
// Six columns travel together through phase 3 -- any six, of whatever joints: each is on its own path (Euler-tour test, as in
// apparent_inertia_kernel), and a body's transform, U and D^-1 are read once for the six.  Phase 2 takes the columns of a group one
// after the other: a path is short against the tree, and a joint climb of six different paths would need the branching bookkeeping of
// an inward sweep.  The arithmetic of a column depends neither on its place in the group nor on its companions: a listed column
// carries the bits of the same column of the full matrix.  H^-1 is symmetric; every entry is computed, none is mirrored.
// Groups are independent after phase 1: gridDim.y waves may share a group of 64 configurations, each redoing phase 1 and taking every
// gridDim.y-th group of columns.  Every entry of the output is written: rows and columns no joint owns as zeros.
#pragma once
#include "mh_response_kernels.h"

namespace mh
{
#define MH_WS(slot) ws[(long)(slot)*ws_stride]

constexpr int MINV_MAX_COLUMNS = 64; // MH_MAX_INVERSE_COLUMNS
constexpr int MINV_GROUP = 6;

template <typename T>
struct MinvArgs
{
   Args<T> a;        // m, B, q and its strides, out = Hinv, ws
   long h_bs, h_es;  // batch / entry strides of Hinv ([nv][n_columns] row-major per configuration)
   const int *info;  // [n][RI_STRIDE]: the Euler tour and the a+ slots of apparent_inertia_kernel
   const int *owner; // [nv]: 8 * engine index of the joint that owns the DoF index + its place among the joint's DoFs; -1: no joint
   const int *zero_ofs, *zero_cols; // GravArgs: zero_cols[zero_ofs[n] .. zero_ofs[n + 1]) are the matrix rows no joint owns
   int slots, a_base, u_base; // as RespArgs
   int n_columns;    // width of a row of Hinv
   int listed;       // 0: column k is DoF index k (n_columns = nv)
   int col[MINV_MAX_COLUMNS]; // listed: the owner[] entry of column k
};

// ---- phase 1: articulated inertias, leaves to root (ForwardDynamicsCalculator.java:1136-1254 without the bias terms =
//      MultiBodyResponseCalculator's use of them, :1206-1238): the factorisation of H along the tree.  One lane's configuration; ws is
//      the lane's workspace, [slot][64 lanes].  This is phase 1 of apparent_inertia_kernel, statement for statement.  It is a copy and
//      not a function both kernels call: with the shared function the compiler scheduled apparent_inertia_kernel differently (fp64: 8 237
//      -> 8 152 lines of ISA), and that kernel's results are pinned bit for bit by its tests.
template <typename T>
MH_DEV void minv_articulated_inertias(const DevModel &m, const T *CB, ciptr meta, ciptr cfg_map, const T *qrow, long q_es, T *ws)
{
   constexpr long ws_stride = 64;
   const S3<T> Z3{T(0), T(0), T(0), T(0), T(0), T(0)};
   ABI<T> Icarry;
   bool have_carry = false;
   for (int j = m.n - 1; j >= 0; j--)
   {
      ciptr mi = meta + j * MI_STRIDE;
      const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
      const bool locked = (flags & MF_LOCKED) != 0;
      const CRef<T> c{CB + j * MC_STRIDE};
      ABI<T> IA = abi_from_rigid(load_inertia<T>(c));
      if (have_carry)
         add(IA, Icarry);
      if (flags & MF_HAS_ACC)
         add(IA, ws_load_abi(ws, ws_stride, mi[MI_SLOT_IA]));
      have_carry = false;
      const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, q_es, ws, ws_stride, mi[MI_SLOT_JP], true);
      ABI<T> Ia = IA;
      bool nothing_up = false;
      if (type == JT_REVOLUTE || type == JT_PRISMATIC)
      {
         V3<T> ua, ul;
         T D;
         if (type == JT_REVOLUTE)
            ua = V3<T>{IA.A.xz, IA.A.yz, IA.A.zz}, ul = V3<T>{IA.C.zx, IA.C.zy, IA.C.zz}, D = IA.A.zz;
         else
            ua = V3<T>{IA.C.xz, IA.C.yz, IA.C.zz}, ul = V3<T>{IA.L.xz, IA.L.yz, IA.L.zz}, D = IA.L.zz;
         const T dinv = locked ? T(0) : T(1) / D;
         const int sf = mi[MI_SLOT_F];
         ws_store6(ws, ws_stride, sf, SV<T>{ua, ul});
         MH_WS(sf + 6) = dinv;
         if (parent >= 0 && !locked)
         {
            if (type == JT_REVOLUTE)
               rank1_down_revolute(Ia, ua, ul, dinv);
            else
               rank1_down(Ia, ua, ul, dinv);
         }
      }
      else if (type == JT_PLANAR || type == JT_SPHERICAL)
      {
         const SV<T> U0 = mul(IA, unit_twist<T>(type, 0)), U1 = mul(IA, unit_twist<T>(type, 1)), U2 = mul(IA, unit_twist<T>(type, 2));
         const V3<T> d0 = comp3(type, U0), d1 = comp3(type, U1), d2 = comp3(type, U2);
         const S3<T> Di = locked ? Z3 : spd3_inverse(S3<T>{d0.x, d0.y, d0.z, d1.y, d1.z, d2.z});
         const int sl = mi[MI_SLOT_LK];
         ws_store6(ws, ws_stride, sl, U0), ws_store6(ws, ws_stride, sl + 6, U1), ws_store6(ws, ws_stride, sl + 12, U2);
         MH_WS(sl + 18) = Di.xx, MH_WS(sl + 19) = Di.xy, MH_WS(sl + 20) = Di.xz, MH_WS(sl + 21) = Di.yy, MH_WS(sl + 22) = Di.yz, MH_WS(sl + 23) = Di.zz;
         if (parent >= 0 && !locked)
         {
            const SV<T> W0 = Di.xx * U0 + Di.xy * U1 + Di.xz * U2, W1 = Di.xy * U0 + Di.yy * U1 + Di.yz * U2, W2 = Di.xz * U0 + Di.yz * U1 + Di.zz * U2;
            rank1_pair_down(Ia, W0, U0), rank1_pair_down(Ia, W1, U1), rank1_pair_down(Ia, W2, U2);
         }
      }
      else if (type == JT_SIXDOF && !locked)
      { // S = 1_6: the change of acceleration is IA^-1 u+ whatever the parent does, and nothing reaches the parent
         const LDL6<T> F = spd6_factor(IA);
         const int sl = mi[MI_SLOT_LK];
#pragma unroll
         for (int k = 0; k < 21; k++)
            MH_WS(sl + k) = F.f[k];
         nothing_up = true;
      }
      if (parent >= 0)
      {
         if (nothing_up)
            Ia.A = Z3, Ia.L = Z3, Ia.C = M3<T>{T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)};
         else
            abi_up(type, jx, load_xb<T>(c), Ia);
         if (flags & MF_PARENT_ADJ)
            Icarry = Ia, have_carry = true;
         else
         {
            ciptr pmi = meta + parent * MI_STRIDE;
            if (flags & MF_ACC_FIRST)
               ws_store_abi(ws, ws_stride, pmi[MI_SLOT_IA], Ia);
            else
            {
               ABI<T> acc = ws_load_abi(ws, ws_stride, pmi[MI_SLOT_IA]);
               add(acc, Ia);
               ws_store_abi(ws, ws_stride, pmi[MI_SLOT_IA], acc);
            }
         }
      }
   }
}

template <typename T>
__global__ void __launch_bounds__(256) mass_matrix_inverse_kernel(MinvArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map), info = as_const(G.info);
   const ciptr owner = as_const(G.owner), zero_ofs = as_const(G.zero_ofs), zero_cols = as_const(G.zero_cols);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)G.slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};
   const int nc = G.n_columns;
   const int groups = (nc + MINV_GROUP - 1) / MINV_GROUP;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      T *Hrow = A.out + cfg * G.h_bs;
      const long h_es = G.h_es;
      minv_articulated_inertias<T>(m, CB, meta, cfg_map, qrow, A.q_es, ws);

      for (int g = part; g < groups; g += parts)
      {
         const int k0 = g * MINV_GROUP, count = min(MINV_GROUP, nc - k0);
         // ---- phase 2: a unit effort at the column's DoF, up its path (:685-735, :1206-1238); one column at a time
         for (int k = 0; k < count; k++)
         {
            const int own = G.listed ? G.col[k0 + k] : owner[k0 + k];
            if (own < 0)
               continue; // no joint owns this DoF index: a column of zeros, u+ is never read (phase 3 finds it on no path)
            const int ec = own >> 3, lc = own & 7;
            SV<T> P{Z, Z};
            for (int e = ec; e >= 0;)
            {
               ciptr mi = meta + e * MI_STRIDE;
               const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
               const int su = G.u_base + 6 * mi[MI_DOF];
               const bool first = e == ec;
               if (type == JT_REVOLUTE || type == JT_PRISMATIC)
               {
                  const int sf = mi[MI_SLOT_F];
                  const SV<T> U = ws_load6(ws, ws_stride, sf);
                  const T dinv = MH_WS(sf + 6);
                  const T u = (first ? T(1) : T(0)) - (type == JT_REVOLUTE ? P.a.z : P.l.z);
                  MH_WS(su + k) = u;
                  P = P + (dinv * u) * U;
               }
               else if (type == JT_PLANAR || type == JT_SPHERICAL)
               {
                  const int sl = mi[MI_SLOT_LK];
                  const SV<T> U0 = ws_load6(ws, ws_stride, sl), U1 = ws_load6(ws, ws_stride, sl + 6), U2 = ws_load6(ws, ws_stride, sl + 12);
                  const S3<T> Di{MH_WS(sl + 18), MH_WS(sl + 19), MH_WS(sl + 20), MH_WS(sl + 21), MH_WS(sl + 22), MH_WS(sl + 23)};
                  const V3<T> e3{first && lc == 0 ? T(1) : T(0), first && lc == 1 ? T(1) : T(0), first && lc == 2 ? T(1) : T(0)};
                  const V3<T> u = e3 - comp3(type, P);
                  MH_WS(su + 3 * k) = u.x, MH_WS(su + 3 * k + 1) = u.y, MH_WS(su + 3 * k + 2) = u.z;
                  const V3<T> x = mul(Di, u);
                  P = P + x.x * U0 + x.y * U1 + x.z * U2;
               }
               else if (type == JT_SIXDOF && !(flags & MF_LOCKED))
               { // a+ of the floating body itself, IA^-1 u+.  U D^-1 = 1_6, so pa+ = pA+ + (e - pA+) = e: the parent feels the reaction
                 // to the unit effort alone (nothing, when the column belongs to a joint further out)
                  LDL6<T> F;
                  const int sl = mi[MI_SLOT_LK];
#pragma unroll
                  for (int i = 0; i < 21; i++)
                     F.f[i] = MH_WS(sl + i);
                  const SV<T> e6{V3<T>{first && lc == 0 ? T(1) : T(0), first && lc == 1 ? T(1) : T(0), first && lc == 2 ? T(1) : T(0)},
                                 V3<T>{first && lc == 3 ? T(1) : T(0), first && lc == 4 ? T(1) : T(0), first && lc == 5 ? T(1) : T(0)}};
                  ws_store6(ws, ws_stride, su + 6 * k, spd6_solve(F, e6 - P));
                  P = e6;
               }
               if (parent >= 0)
                  P = force_up(type, joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]),
                               load_xb<T>(CRef<T>{CB + e * MC_STRIDE}), P);
               e = parent;
            }
         }
         // ---- phase 3: change of acceleration of every body, root outwards (:1259-1338); the joint's share of it is the entry
         int tin_c[MINV_GROUP], tout_c[MINV_GROUP]; // the Euler tour of each column's joint; (-1, -1): on nobody's path
#pragma unroll
         for (int k = 0; k < MINV_GROUP; k++)
         {
            const int own = k < count ? (G.listed ? G.col[k0 + k] : owner[k0 + k]) : -1;
            tin_c[k] = own < 0 ? -1 : info[(own >> 3) * RI_STRIDE + RI_TIN];
            tout_c[k] = own < 0 ? -1 : info[(own >> 3) * RI_STRIDE + RI_TOUT];
         }
         SV<T> ac[MINV_GROUP]; // a+ of the body visited last, one per column
#pragma unroll
         for (int k = 0; k < MINV_GROUP; k++)
            ac[k] = SV<T>{Z, Z};
         for (int j = 0; j < m.n; j++)
         {
            ciptr mi = meta + j * MI_STRIDE;
            const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
            const int tin = info[j * RI_STRIDE + RI_TIN], tout = info[j * RI_STRIDE + RI_TOUT];
            bool on_path[MINV_GROUP]; // the column's joint lies in the subtree of j
#pragma unroll
            for (int k = 0; k < MINV_GROUP; k++)
               on_path[k] = tin <= tin_c[k] && tout_c[k] <= tout;
            const int su = G.u_base + 6 * mi[MI_DOF];
            ciptr dj = dof_map + mi[MI_DOF];
            T *o = Hrow + (long)k0 * h_es; // + (row * nc + k) * h_es
            if (parent < 0)
            {
#pragma unroll
               for (int k = 0; k < MINV_GROUP; k++)
                  ac[k] = SV<T>{Z, Z};
            }
            else
            {
               if (!(flags & MF_PARENT_ADJ))
               {
                  const int sp = G.a_base + info[parent * RI_STRIDE + RI_SLOT_A];
#pragma unroll
                  for (int k = 0; k < MINV_GROUP; k++)
                     ac[k] = ws_load6(ws, ws_stride, sp + 6 * k);
               }
               const XF<T> Xb = load_xb<T>(CRef<T>{CB + j * MC_STRIDE});
               const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
#pragma unroll
               for (int k = 0; k < MINV_GROUP; k++)
                  ac[k] = motion_down(type, jx, Xb, ac[k]);
            }
            if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            {
               const int sf = mi[MI_SLOT_F];
               const SV<T> U = ws_load6(ws, ws_stride, sf);
               const T dinv = MH_WS(sf + 6);
               const long row = (long)dj[0] * nc;
#pragma unroll
               for (int k = 0; k < MINV_GROUP; k++)
               {
                  const T u = on_path[k] ? MH_WS(su + k) : T(0);
                  const T qdd = dinv * (u - dot6(U, ac[k]));
                  if (type == JT_REVOLUTE)
                     ac[k].a.z += qdd;
                  else
                     ac[k].l.z += qdd;
                  if (k < count)
                     o[(row + k) * h_es] = qdd;
               }
            }
            else if (type == JT_PLANAR || type == JT_SPHERICAL)
            {
               const int sl = mi[MI_SLOT_LK];
               const SV<T> U0 = ws_load6(ws, ws_stride, sl), U1 = ws_load6(ws, ws_stride, sl + 6), U2 = ws_load6(ws, ws_stride, sl + 12);
               const S3<T> Di{MH_WS(sl + 18), MH_WS(sl + 19), MH_WS(sl + 20), MH_WS(sl + 21), MH_WS(sl + 22), MH_WS(sl + 23)};
               const long r0 = (long)dj[0] * nc, r1 = (long)dj[1] * nc, r2 = (long)dj[2] * nc;
#pragma unroll
               for (int k = 0; k < MINV_GROUP; k++)
               {
                  V3<T> u = Z;
                  if (on_path[k])
                     u = V3<T>{MH_WS(su + 3 * k), MH_WS(su + 3 * k + 1), MH_WS(su + 3 * k + 2)};
                  const V3<T> r = u - V3<T>{dot6(U0, ac[k]), dot6(U1, ac[k]), dot6(U2, ac[k])};
                  const V3<T> qdd = mul(Di, r);
                  ac[k] = ac[k] + from_comp3(type, qdd);
                  if (k < count)
                     o[(r0 + k) * h_es] = qdd.x, o[(r1 + k) * h_es] = qdd.y, o[(r2 + k) * h_es] = qdd.z;
               }
            }
            else if (type == JT_SIXDOF)
            { // S = 1_6: qdd+ = a+ - X a+_parent with a+ = IA^-1 u+; an ACCELERATION_SOURCE floating joint follows its parent, qdd+ = 0
               const bool locked = (flags & MF_LOCKED) != 0;
#pragma unroll
               for (int k = 0; k < MINV_GROUP; k++)
               {
                  SV<T> qdd{Z, Z};
                  if (!locked)
                  {
                     const SV<T> x = on_path[k] ? ws_load6(ws, ws_stride, su + 6 * k) : SV<T>{Z, Z};
                     qdd = x - ac[k];
                     ac[k] = x;
                  }
                  if (k < count)
                  {
                     o[((long)dj[0] * nc + k) * h_es] = qdd.a.x, o[((long)dj[1] * nc + k) * h_es] = qdd.a.y;
                     o[((long)dj[2] * nc + k) * h_es] = qdd.a.z, o[((long)dj[3] * nc + k) * h_es] = qdd.l.x;
                     o[((long)dj[4] * nc + k) * h_es] = qdd.l.y, o[((long)dj[5] * nc + k) * h_es] = qdd.l.z;
                  }
               }
            }
            const int sa = info[j * RI_STRIDE + RI_SLOT_A];
            if (sa >= 0)
               resp_store_cols(ws, ws_stride, G.a_base + sa, ac);
         }
         // matrix rows no joint owns
         for (int z = zero_ofs[m.n]; z < zero_ofs[m.n + 1]; z++)
            for (int k = 0; k < count; k++)
               Hrow[((long)zero_cols[z] * nc + k0 + k) * h_es] = T(0);
      }
   }
}

#undef MH_WS
} // namespace mh
