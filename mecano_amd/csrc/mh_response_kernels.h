// mh_response_kernels.h -- inverse apparent inertia of bodies: how target body b accelerates when a unit wrench acts on target body a
// (run-time topology, one lane per configuration, gfx950).
//
// Replaces, per configuration, algorithms/MultiBodyResponseCalculator.java:288-440 (computeRigidBodyApparentSpatialInertiaInverse),
// :608-627 / :859-862 (applyRigidBodyWrench, the acceleration change provider) and the recursion behind them, :1191-1338, in the engine's
// canonical joint frames.  For K targets the blocks W_ba (6 x 6) of W = J H^-1 J^T come out of the articulated-body recursion itself;
// neither J nor H is formed:
//   1. inward sweep over all bodies, configuration only: articulated inertia IA, U = IA S and D^-1 of every joint, kept in the
//      workspace slots the forward-dynamics kernel keeps them in (MI_SLOT_F: U, D^-1; MI_SLOT_LK: U, D^-1 of a 3-DoF joint or the LDL^T
//      factor of a floating joint's IA).  No velocities, efforts or bias terms.  An ACCELERATION_SOURCE joint hands IA up undiminished and
//      gets D^-1 = 0, which makes its change of acceleration zero in the two phases below without a branch (:1230-1238, 1275-1281).
//   2. per source a: the six unit wrenches of its frame as test wrenches pA+ = -X_a^T w, climbed to the root (u+ = -S^T pA+,
//      pa+ = pA+ + U D^-1 u+, force transform), u+ of the six columns kept per joint of the path.
//   3. back down over the bodies that have a target in their subtree (COUPLED) or the source in it (DIAGONAL):
//      qdd+ = D^-1 (u+ - U^T a+_parent), u+ = 0 off the source's path, a+ = X a+_parent + S qdd+; at target b the six columns of a+,
//      brought to b's frame, are block (b, a).
// The six columns of a source are carried together (a 6 x 6 block in registers: the joint's transform, U and D^-1 are read once per
// body).  Which bodies take part is decided on the device from the Euler tour of the tree (a constant of the model) and the targets in
// the kernel arguments: the call has no plan to upload.  Sources are independent after phase 1: gridDim.y waves may share a group of
// 64 configurations, each redoing phase 1 and taking every gridDim.y-th source.
#pragma once
#include "mh_kernels.h"

namespace mh
{
#define MH_WS(slot) ws[(long)(slot)*ws_stride]

constexpr int RESP_MAX_TARGETS = 16; // MH_MAX_APPARENT_TARGETS
enum : int
{
   RI_TIN = 0,    // Euler tour of the tree: body x lies in the subtree of j  <=>  tin[j] <= tin[x] && tout[x] <= tout[j]
   RI_TOUT = 1,
   RI_SLOT_A = 2, // 36 slots for a+ of a body some child of which does not directly follow it (-1: none), relative to RespArgs::a_base
   RI_STRIDE = 4
};

template <typename T>
struct RespArgs
{
   Args<T> a;      // m, B, q and its strides, out = W, ws
   long w_bs, w_es; // batch / entry strides of W
   const int *info; // [n][RI_STRIDE]
   int slots;      // workspace slots per lane: those of the model, then 36 per RI_SLOT_A body (a_base), then 6 per DoF (u_base)
   int a_base, u_base;
   int n_targets, coupled;
   int tgt[RESP_MAX_TARGETS];      // engine index of every target's body
   T pose[RESP_MAX_TARGETS][12];   // the target frame in the body's canonical after-joint frame (R row-major, p)
};

template <typename T>
MH_DEV void resp_store_cols(T *ws, long ws_stride, int slot, const SV<T> (&a)[6])
{
#pragma unroll
   for (int k = 0; k < 6; k++)
      ws_store6(ws, ws_stride, slot + 6 * k, a[k]);
}
template <typename T>
MH_DEV T dot6(const SV<T> &u, const SV<T> &a)
{
   return u.a.x * a.a.x + u.a.y * a.a.y + u.a.z * a.a.z + u.l.x * a.l.x + u.l.y * a.l.y + u.l.z * a.l.z;
}

template <typename T>
__global__ void __launch_bounds__(256) apparent_inertia_kernel(RespArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map), info = as_const(G.info);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)G.slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};
   const S3<T> Z3{T(0), T(0), T(0), T(0), T(0), T(0)};
   const int K = G.n_targets;
   const long ld = G.coupled ? 6L * K : 6L;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      T *Wrow = A.out + cfg * G.w_bs;
      const long w_es = G.w_es;
      // ---- phase 1: articulated inertias, leaves to root (ForwardDynamicsCalculator.java:1136-1254 without the bias terms =
      //      MultiBodyResponseCalculator's use of them, :1206-1238)
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
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP], true);
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

      for (int a = part; a < K; a += parts)
      {
         const int ea = G.tgt[a];
         const int tin_a = info[ea * RI_STRIDE + RI_TIN], tout_a = info[ea * RI_STRIDE + RI_TOUT];
         // ---- phase 2: the six unit wrenches of the source's frame, up its path (:1206-1238)
         SV<T> P[6];
         {
            const T *ps = G.pose[a];
            const XF<T> Xa{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
#pragma unroll
            for (int k = 0; k < 6; k++)
            {
               SV<T> w{Z, Z};
               (k == 0 ? w.a.x : k == 1 ? w.a.y : k == 2 ? w.a.z : k == 3 ? w.l.x : k == 4 ? w.l.y : w.l.z) = T(-1);
               P[k] = force_to_parent(Xa, w);
            }
         }
         for (int e = ea; e >= 0;)
         {
            ciptr mi = meta + e * MI_STRIDE;
            const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
            const int su = G.u_base + 6 * mi[MI_DOF];
            if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            {
               const int sf = mi[MI_SLOT_F];
               const SV<T> U = ws_load6(ws, ws_stride, sf);
               const T dinv = MH_WS(sf + 6);
#pragma unroll
               for (int k = 0; k < 6; k++)
               {
                  const T u = T(0) - (type == JT_REVOLUTE ? P[k].a.z : P[k].l.z);
                  MH_WS(su + k) = u;
                  P[k] = P[k] + (dinv * u) * U;
               }
            }
            else if (type == JT_PLANAR || type == JT_SPHERICAL)
            {
               const int sl = mi[MI_SLOT_LK];
               const SV<T> U0 = ws_load6(ws, ws_stride, sl), U1 = ws_load6(ws, ws_stride, sl + 6), U2 = ws_load6(ws, ws_stride, sl + 12);
               const S3<T> Di{MH_WS(sl + 18), MH_WS(sl + 19), MH_WS(sl + 20), MH_WS(sl + 21), MH_WS(sl + 22), MH_WS(sl + 23)};
#pragma unroll
               for (int k = 0; k < 6; k++)
               {
                  const V3<T> u = Z - comp3(type, P[k]);
                  MH_WS(su + 3 * k) = u.x, MH_WS(su + 3 * k + 1) = u.y, MH_WS(su + 3 * k + 2) = u.z;
                  const V3<T> x = mul(Di, u);
                  P[k] = P[k] + x.x * U0 + x.y * U1 + x.z * U2;
               }
            }
            else if (type == JT_SIXDOF && !(flags & MF_LOCKED))
            {
               LDL6<T> F;
               const int sl = mi[MI_SLOT_LK];
#pragma unroll
               for (int k = 0; k < 21; k++)
                  F.f[k] = MH_WS(sl + k);
#pragma unroll
               for (int k = 0; k < 6; k++)
               { // a+ of the floating body itself; its parent feels nothing
                  ws_store6(ws, ws_stride, su + 6 * k, spd6_solve(F, SV<T>{Z, Z} - P[k]));
                  P[k] = SV<T>{Z, Z};
               }
            }
            if (parent >= 0)
            {
               const XF<T> Xb = load_xb<T>(CRef<T>{CB + e * MC_STRIDE});
               const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
#pragma unroll
               for (int k = 0; k < 6; k++)
                  P[k] = force_up(type, jx, Xb, P[k]);
            }
            e = parent;
         }
         // ---- phase 3: change of acceleration, root to the targets (:1259-1338)
         SV<T> ac[6]; // a+ of the body visited last, six columns
#pragma unroll
         for (int k = 0; k < 6; k++)
            ac[k] = SV<T>{Z, Z};
         for (int j = 0; j < m.n; j++)
         {
            const int tin = info[j * RI_STRIDE + RI_TIN], tout = info[j * RI_STRIDE + RI_TOUT];
            const bool on_path = tin <= tin_a && tout_a <= tout; // the source lies in the subtree of j
            bool wanted = on_path;
            for (int b = 0; G.coupled && !wanted && b < K; b++)
            {
               const int tb = info[G.tgt[b] * RI_STRIDE + RI_TIN];
               wanted = tin <= tb && tb <= tout;
            }
            if (!wanted)
               continue;
            ciptr mi = meta + j * MI_STRIDE;
            const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
            const int su = G.u_base + 6 * mi[MI_DOF];
            if (parent < 0)
            {
#pragma unroll
               for (int k = 0; k < 6; k++)
                  ac[k] = SV<T>{Z, Z};
            }
            else
            {
               if (!(flags & MF_PARENT_ADJ))
               {
                  const int sp = G.a_base + info[parent * RI_STRIDE + RI_SLOT_A];
#pragma unroll
                  for (int k = 0; k < 6; k++)
                     ac[k] = ws_load6(ws, ws_stride, sp + 6 * k);
               }
               const XF<T> Xb = load_xb<T>(CRef<T>{CB + j * MC_STRIDE});
               const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
#pragma unroll
               for (int k = 0; k < 6; k++)
                  ac[k] = motion_down(type, jx, Xb, ac[k]);
            }
            if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            {
               const int sf = mi[MI_SLOT_F];
               const SV<T> U = ws_load6(ws, ws_stride, sf);
               const T dinv = MH_WS(sf + 6);
#pragma unroll
               for (int k = 0; k < 6; k++)
               {
                  const T u = on_path ? MH_WS(su + k) : T(0);
                  const T qdd = dinv * (u - dot6(U, ac[k]));
                  if (type == JT_REVOLUTE)
                     ac[k].a.z += qdd;
                  else
                     ac[k].l.z += qdd;
               }
            }
            else if (type == JT_PLANAR || type == JT_SPHERICAL)
            {
               const int sl = mi[MI_SLOT_LK];
               const SV<T> U0 = ws_load6(ws, ws_stride, sl), U1 = ws_load6(ws, ws_stride, sl + 6), U2 = ws_load6(ws, ws_stride, sl + 12);
               const S3<T> Di{MH_WS(sl + 18), MH_WS(sl + 19), MH_WS(sl + 20), MH_WS(sl + 21), MH_WS(sl + 22), MH_WS(sl + 23)};
#pragma unroll
               for (int k = 0; k < 6; k++)
               {
                  V3<T> u = Z;
                  if (on_path)
                     u = V3<T>{MH_WS(su + 3 * k), MH_WS(su + 3 * k + 1), MH_WS(su + 3 * k + 2)};
                  const V3<T> r = u - V3<T>{dot6(U0, ac[k]), dot6(U1, ac[k]), dot6(U2, ac[k])};
                  ac[k] = ac[k] + from_comp3(type, mul(Di, r));
               }
            }
            else if (type == JT_SIXDOF && !(flags & MF_LOCKED))
            {
#pragma unroll
               for (int k = 0; k < 6; k++)
                  ac[k] = on_path ? ws_load6(ws, ws_stride, su + 6 * k) : SV<T>{Z, Z};
            }
            const int sa = info[j * RI_STRIDE + RI_SLOT_A];
            if (sa >= 0)
               resp_store_cols(ws, ws_stride, G.a_base + sa, ac);
            // block (b, a) of every target b on this body: the columns in b's frame
            for (int b = 0; b < K; b++)
            {
               if (G.tgt[b] != j || !(G.coupled || b == a))
                  continue;
               const T *pb = G.pose[b];
               const XF<T> Xt{M3<T>{pb[0], pb[1], pb[2], pb[3], pb[4], pb[5], pb[6], pb[7], pb[8]}, V3<T>{pb[9], pb[10], pb[11]}};
               const long row0 = G.coupled ? 6L * b * ld + 6L * a : 36L * b;
#pragma unroll
               for (int k = 0; k < 6; k++)
               {
                  const SV<T> v = motion_to_child(Xt, ac[k]);
                  T *o = Wrow + (row0 + k) * w_es;
                  o[0 * ld * w_es] = v.a.x, o[1 * ld * w_es] = v.a.y, o[2 * ld * w_es] = v.a.z;
                  o[3 * ld * w_es] = v.l.x, o[4 * ld * w_es] = v.l.y, o[5 * ld * w_es] = v.l.z;
               }
            }
         }
      }
   }
}

#undef MH_WS
} // namespace mh
