// mh_rnea_vjp_kernels.h -- reverse-mode gradients of the inverse dynamics: for a cotangent u of the efforts, u^T d tau / d q, u^T d tau / d qd
// and H u of every configuration (run-time topology, one lane per configuration, gfx950).  The matrices are those of
// rnea_derivatives_kernel (mh_rnea_deriv_kernels.h, whose notation this file keeps): the same velocity-space chart, the same fixed
// components of qd and qdd, wrenches held in the world -- but none of them is formed, and nothing climbs.
//
// Column (j, k) of a matrix holds the entries of joint j's own rows (S_r . P, S_r . Q), of its ancestors' rows (S_r . P' and S_r . Q with
// P', Q climbed as forces) and of its descendants' rows (the climbed T1, T4, T5 of the descendant's DoF, picked at j).  Contracted with u:
//   own rows          (S_j u_j) . P                                            S_j u_j = sum_k u_jk S_jk
//   ancestors' rows   sum_a (S_a u_a) . force_up_{j -> a}(P') = nul_j . P'      motion_down is the adjoint of force_up; nul_j = the sum of
//                     the ancestors' S_a u_a brought down to frame j = nu_j - S_j u_j with nu_j = motion_down(nu_parent) + S_j u_j
//   descendants' rows T1, T4, T5 are linear in the descendant's twist, so the sums over the strict descendants d, in frame j,
//                        T1b = sum Ic_d (S_d u_d),   T4b = sum BSc_d^T (S_d u_d),   T5b = -sum (S_d u_d) x* Wc_d
//                     are three more composites of the inward sweep: every body hands T?b + its own term to its parent with force_up.
// Per DoF (j, k), s = S_jk, that is
//   gq [jk]  = (S_j u_j) . P + nul_j . (P + s x* Fc) + s . (T5b - vl x* (T4b - vl x* T1b) - al x* T1b)
//   gqd[jk]  = (S_j u_j + nul_j) . Q                 + s . (T4b - (vl + v) x* T1b)
//   gqdd[jk] = s . (Ic nu_j + T1b)                    = (H u)[jk]: nu_j is the acceleration of body j for qdd = u at rest without gravity,
//              Ic nu_j the force of the subtree moving with j, T1b what the descendants' own joints add
// and the dot products with P and Q turn into components as well: Ic is symmetric, m . (BSc x) = x . (BSc^T m), and
// m . (v x s) = -s . (v x* m), (s x* f) . m = -s . (m x* f).  With
//   X1 = T1b + Ic nu,   X4 = T4b + BSc^T nu,   X5 = T5b - nu x* Wc - nul x* Fc
// every entry is one component of a vector formed once per body -- the row of an ancestor, of the joint itself and of a descendant meet
// in the same three sums:
//   gq [jk] = s . (X5 - vl x* (X4 - vl x* X1) - al x* X1),   gqd[jk] = s . (X4 - (vl + v) x* X1),   gqdd[jk] = s . X1
// Two sweeps, O(n), no loop over DoF pairs; every output entry is written once, by the wave that owns the body (j % parts == part), no
// atomics.  u = 0 gives exact zeros, qd = 0 (consider_coriolis = 0) exact zeros in gqd.
// rnea_parameters_state_vjp_kernel (mh_params_state_vjp_kernels.h) holds a copy of both sweeps with the inertia taken from the lane's own
// parameters: a change to a sweep here is made there too.
#pragma once
#include "mh_rnea_deriv_kernels.h"
#include "mh_response_kernels.h" // dot6

namespace mh
{
// workspace slots of a body, from VjpArgs::slot[j] (vjp_slot_plan, mh_launch_plans.h)
enum : int
{
   VS_JP = 0,   // 2: (cos, sin) of a revolute joint
   VS_F = 2,    // 6: body force, then the subtree's (children add theirs)
   VS_VL = 8,   // 6: the parent's velocity in this frame
   VS_AL = 14,  // 6: the parent's acceleration in this frame
   VS_V = 20,   // 6: velocity
   VS_W = 26,   // 6: external force, then the subtree's
   VS_H = 32,   // 6: momentum, then the subtree's
   VS_NUL = 38, // 6: nul, the ancestors' S u in this frame
   VS_BC = 44,  // 30: composite factorised inertia of the children (handed through the workspace by every child, as DS_BC is)
   VS_BODY = 74,
   // bodies with a child that does not directly follow them (MF_STORE_VA) only:
   VS_A = 74,   // 6: acceleration, for those children
   VS_NU = 80,  // 6: nu, for those children
   VS_IC = 86,  // 10: composite inertia accumulator
   VS_T1 = 96,  // 6 + 6 + 6: T1b, T4b, T5b of those children (zeroed on the way out, added to on the way in)
   VS_T4 = 102,
   VS_T5 = 108,
   VS_BRANCH = 114
};

template <typename T>
struct VjpArgs
{
   Args<T> a;           // m, B, q, qd, in3 = qdd (read only with accel), fext (or NULL), root acceleration, the switches; out is not used
   const T *u;          // [nv] cotangent of the efforts, strides of qd
   T *gq, *gqd, *gqdd;  // [nv] each, strides of qd; any may be NULL
   const int *slot;     // [n] first workspace slot of every body
   int slots;           // workspace slots per lane
   int negate;          // store -gq and -gqd (the forward form: u = H^-1 w)
   int accumulate;      // gq and gqd are added to what the outputs hold (mh_aba_integrate_vjp_*); unowned entries are left alone
   const int *unowned;  // DoF indices no joint owns: zeros
   int n_unowned;
};

template <typename T>
__global__ void __launch_bounds__(256) rnea_vjp_kernel(VjpArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const ciptr slot = as_const(G.slot), unowned = as_const(G.unowned);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   // gridDim.y waves may share a group of 64 configurations (small batches): each runs the sweeps and stores the entries of every
   // gridDim.y-th body
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)G.slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};
   const SV<T> Z6{Z, Z};
   const bool with_ext = A.fext != nullptr, with_gq = G.gq != nullptr, with_gqd = G.gqd != nullptr, with_gqdd = G.gqdd != nullptr;
   const T sign = G.negate ? T(-1) : T(1);
   const bool acc = G.accumulate != 0;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *qddrow = A.in3 + cfg * A.v_bs;
      const T *urow = G.u + cfg * A.v_bs;
      const T *frow = with_ext ? A.fext + cfg * A.f_bs : nullptr;
      T *gq = with_gq ? G.gq + cfg * A.v_bs : nullptr;
      T *gqd = with_gqd ? G.gqd + cfg * A.v_bs : nullptr;
      T *gqdd = with_gqdd ? G.gqdd + cfg * A.v_bs : nullptr;
      // ---- outward sweep: velocities, accelerations, the Newton-Euler force and the momentum of every body; nu beside them
      SV<T> v_prev = Z6, a_prev = Z6, nu_prev = Z6;
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int s = slot[j];
         SV<T> vp, ap, nup;
         if (parent < 0)
            vp = Z6, ap = root_acceleration(A), nup = Z6;
         else if (flags & MF_PARENT_ADJ)
            vp = v_prev, ap = a_prev, nup = nu_prev;
         else
         {
            const int sp = slot[parent];
            vp = ws_load6(ws, ws_stride, sp + VS_V);
            ap = ws_load6(ws, ws_stride, sp + VS_A);
            nup = ws_load6(ws, ws_stride, sp + VS_NU);
         }
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, s + VS_JP, true);
         const SV<T> vJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, A.coriolis != 0);
         const SV<T> aJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qddrow, A.v_es, A.accel != 0);
         const SV<T> Su = joint_vec<T>(type, dof_map, mi[MI_DOF], urow, A.v_es, true);
         const SV<T> vl = motion_down(type, jx, Xb, vp), al = motion_down(type, jx, Xb, ap), nul = motion_down(type, jx, Xb, nup);
         const SV<T> v = vl + vJ;
         const SV<T> a = al + aJ + crm(v, vJ);
         const SV<T> nu = nul + Su;
         const RI<T> I = load_inertia<T>(c);
         const SV<T> h = mul(I, v);
         SV<T> f = mul(I, a) + crf(v, h);
         if (with_ext)
         {
            const SV<T> fe = load_fext<T>(c, frow, A.f_es, mi[MI_EXT]);
            f = f - fe;
            ws_store6(ws, ws_stride, s + VS_W, fe);
         }
         ws_store6(ws, ws_stride, s + VS_F, f);
         ws_store6(ws, ws_stride, s + VS_VL, vl);
         ws_store6(ws, ws_stride, s + VS_AL, al);
         ws_store6(ws, ws_stride, s + VS_V, v);
         ws_store6(ws, ws_stride, s + VS_H, h);
         ws_store6(ws, ws_stride, s + VS_NUL, nul);
         if (flags & MF_STORE_VA)
         {
            ws_store6(ws, ws_stride, s + VS_A, a);
            ws_store6(ws, ws_stride, s + VS_NU, nu);
            ws_store6(ws, ws_stride, s + VS_T1, Z6);
            ws_store6(ws, ws_stride, s + VS_T4, Z6);
            ws_store6(ws, ws_stride, s + VS_T5, Z6);
         }
         v_prev = v, a_prev = a, nu_prev = nu;
      }
      // ---- inward sweep: the composites, and the entries of the body's DoFs
      RI<T> rcarry;
      SV<T> fcarry = Z6, wcarry = Z6, hcarry = Z6, t1carry = Z6, t4carry = Z6, t5carry = Z6;
      bool have_carry = false;
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int s = slot[j];
         const SV<T> vj = ws_load6(ws, ws_stride, s + VS_V);
         RI<T> Ic = load_inertia<T>(c);
         FB<T> Bc = fb_from_rigid(Ic, vj);
         SV<T> F = ws_load6(ws, ws_stride, s + VS_F), h = ws_load6(ws, ws_stride, s + VS_H), W = Z6;
         SV<T> T1 = Z6, T4 = Z6, T5 = Z6;
         if (with_ext)
            W = ws_load6(ws, ws_stride, s + VS_W);
         if (have_carry)
         {
            add(Ic, rcarry);
            F = F + fcarry, h = h + hcarry, W = W + wcarry;
            T1 = t1carry, T4 = t4carry, T5 = t5carry;
         }
         if (flags & MF_HAS_ACC)
         {
            add(Ic, ws_load_ri(ws, ws_stride, s + VS_IC));
            T1 = T1 + ws_load6(ws, ws_stride, s + VS_T1);
            T4 = T4 + ws_load6(ws, ws_stride, s + VS_T4);
            if (with_ext)
               T5 = T5 + ws_load6(ws, ws_stride, s + VS_T5);
         }
         if (have_carry || (flags & MF_HAS_ACC))
            add(Bc, ws_load_fb(ws, ws_stride, s + VS_BC));
         have_carry = false;
         const SV<T> Su = joint_vec<T>(type, dof_map, mi[MI_DOF], urow, A.v_es, true);
         // the entries of this body's DoFs first: what they need is dead before the hand-over below makes its copies
         const int nd = dof_count(type);
         if (j % parts == part && nd > 0)
         {
            const SV<T> nul = ws_load6(ws, ws_stride, s + VS_NUL);
            const SV<T> nu = nul + Su;
            const SV<T> X1 = T1 + mul(Ic, nu);
            ciptr dj = dof_map + mi[MI_DOF];
            if (with_gqdd)
               for (int k = 0; k < nd; k++)
                  gqdd[(long)dj[k] * A.v_es] = comp(X1, dof_comp(type, k));
            if (with_gq || with_gqd)
            {
               const SV<T> vl = ws_load6(ws, ws_stride, s + VS_VL);
               const SV<T> X4 = T4 + bs_tmul(Bc, h, nu);
               if (with_gqd)
               {
                  const SV<T> Gv = X4 - crf(vl + vj, X1);
                  for (int k = 0; k < nd; k++)
                  {
                     T *at = gqd + (long)dj[k] * A.v_es;
                     const T val = sign * comp(Gv, dof_comp(type, k));
                     *at = acc ? *at + val : val;
                  }
               }
               if (with_gq)
               {
                  const SV<T> al = ws_load6(ws, ws_stride, s + VS_AL);
                  SV<T> X5 = T5 - crf(nul, F);
                  if (with_ext)
                     X5 = X5 - crf(nu, W);
                  const SV<T> Gq = X5 - crf(vl, X4 - crf(vl, X1)) - crf(al, X1);
                  for (int k = 0; k < nd; k++)
                  {
                     T *at = gq + (long)dj[k] * A.v_es;
                     const T val = sign * comp(Gq, dof_comp(type, k));
                     *at = acc ? *at + val : val;
                  }
               }
            }
         }
         // hand the composites to the parent
         if (parent >= 0)
         {
            const XF<T> Xb = load_xb<T>(c);
            const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, s + VS_JP);
            const SV<T> T1u = force_up(type, jx, Xb, T1 + mul(Ic, Su)), T4u = force_up(type, jx, Xb, T4 + bs_tmul(Bc, h, Su));
            SV<T> Wu = Z6, T5u = Z6;
            if (with_ext)
            {
               Wu = force_up(type, jx, Xb, W);
               T5u = force_up(type, jx, Xb, T5 - crf(Su, W));
            }
            const SV<T> Fu = force_up(type, jx, Xb, F), hu = force_up(type, jx, Xb, h);
            rigid_up(type, jx, Xb, Ic);
            fb_up(type, jx, Xb, Bc);
            const int sp = slot[parent];
            // Bc: the first child to arrive stores, the others add -- the child that directly follows its parent arrives last
            if ((flags & MF_ACC_FIRST) || ((flags & MF_PARENT_ADJ) && !(meta[parent * MI_STRIDE + MI_FLAGS] & MF_HAS_ACC)))
               ws_store_fb(ws, ws_stride, sp + VS_BC, Bc);
            else
            {
               FB<T> bacc = ws_load_fb(ws, ws_stride, sp + VS_BC);
               add(bacc, Bc);
               ws_store_fb(ws, ws_stride, sp + VS_BC, bacc);
            }
            if (flags & MF_PARENT_ADJ)
            {
               rcarry = Ic, fcarry = Fu, hcarry = hu, wcarry = Wu, have_carry = true;
               t1carry = T1u, t4carry = T4u, t5carry = T5u;
            }
            else
            {
               if (flags & MF_ACC_FIRST)
                  ws_store_ri(ws, ws_stride, sp + VS_IC, Ic);
               else
               {
                  RI<T> acc = ws_load_ri(ws, ws_stride, sp + VS_IC);
                  add(acc, Ic);
                  ws_store_ri(ws, ws_stride, sp + VS_IC, acc);
               }
               ws_add6(ws, ws_stride, sp + VS_F, Fu);
               ws_add6(ws, ws_stride, sp + VS_H, hu);
               ws_add6(ws, ws_stride, sp + VS_T1, T1u);
               ws_add6(ws, ws_stride, sp + VS_T4, T4u);
               if (with_ext)
               {
                  ws_add6(ws, ws_stride, sp + VS_W, Wu);
                  ws_add6(ws, ws_stride, sp + VS_T5, T5u);
               }
            }
         }
      }
      // entries no joint owns
      if (part == 0 && !acc)
         for (int z = 0; z < G.n_unowned; z++)
         {
            const long at = (long)unowned[z] * A.v_es;
            if (with_gq)
               gq[at] = T(0);
            if (with_gqd)
               gqd[at] = T(0);
            if (with_gqdd)
               gqdd[at] = T(0);
         }
   }
}

} // namespace mh
