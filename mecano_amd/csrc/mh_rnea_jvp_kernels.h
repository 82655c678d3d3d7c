// mh_rnea_jvp_kernels.h -- forward-mode derivatives of the inverse dynamics: for directions (dq, dqd, dqdd) of every configuration,
//   dtau = (d tau / d q) dq + (d tau / d qd) dqd + H dqdd
// (run-time topology, one lane per configuration, gfx950).  The matrices are those of rnea_derivatives_kernel (mh_rnea_deriv_kernels.h)
// and of rnea_vjp_kernel (mh_rnea_vjp_kernels.h, whose notation this file keeps): dq is a velocity-space step, the components of qd and
// qdd move by plain increments, wrenches are held in the world -- but no matrix is formed.
//
// The kernel is the tangent of the Newton-Euler recursion in body coordinates.  A step S dq_j of joint j moves the frame of body j against
// its parent, so whatever comes down from the parent turns by it (d motion_down(x) = motion_down(dx) + x_local x S dq_j) and whatever goes
// up from a child turns back (d force_up(F) = force_up(dF + (S dq_c) x* F)); the joint's own S is constant in its frame.  With vl, al the
// parent's velocity and acceleration in this frame, vJ = S qd_j and F the subtree's force:
//   outward  xi  = motion_down(xi_p) + S dq_j                         the displacement twist of body j (zero above the root)
//            dvl = motion_down(dv_p) + vl x S dq_j                    dv = dvl + S dqd_j
//            dal = motion_down(da_p) + al x S dq_j                    da = dal + S dqdd_j + dv x vJ + v x S dqd_j   (da_p = 0 above the root)
//            df  = I da + dv x* (I v) + v x* (I dv) + xi x* fe        (a wrench stays where it is in the world: it turns by -xi in the body)
//   inward   dF_j = df_j + sum over the children c of force_up_c(dF_c + (S dq_c) x* F_c),        dtau_j = S_j^T dF_j
// Two sweeps, O(n), nv numbers per configuration written once, by the wave that owns the body (j % parts == part); no atomics.  Zero
// directions give exact zeros; qd = 0 (consider_coriolis = 0) leaves dqd without effect, and it is not read.
// With rhs set the store is tau_in - dtau (-dtau without a tau_in): at dqdd = 0 the right-hand side of the forward form (mh_aba_jvp_*).
#pragma once
#include "mh_kernels.h"

namespace mh
{
// workspace slots of a body, from JvpArgs::slot[j] (jvp_slot_plan, mh_launch_plans.h)
enum : int
{
   JS_JP = 0,   // 2: (cos, sin) of a revolute joint
   JS_F = 2,    // 6: body force, then the subtree's (children add theirs)
   JS_DF = 8,   // 6: its tangent, likewise
   JS_BODY = 14,
   // bodies with a child that does not directly follow them (MF_STORE_VA) only, for those children:
   JS_V = 14,   // 6: velocity
   JS_A = 20,   // 6: acceleration
   JS_XI = 26,  // 6: displacement twist
   JS_DV = 32,  // 6: tangent of the velocity
   JS_DA = 38,  // 6: tangent of the acceleration
   JS_BRANCH = 44
};

template <typename T>
struct JvpArgs
{
   Args<T> a;              // m, B, q, qd, in3 = qdd (read only with accel), fext (or NULL), root acceleration, the switches; out = dtau
   const T *dq, *dqd, *dqdd; // [nv] directions, strides of qd; any may be NULL (zero, not read); dqd is not read without coriolis
   int rhs;                // the store is tau_in - dtau (the forward form)
   const T *tau_in;        // with rhs: [nv], or NULL for zero (not read)
   const int *slot;        // [n] first workspace slot of every body
   int slots;              // workspace slots per lane
   const int *unowned;     // DoF indices no joint owns: zeros
   int n_unowned;
};

template <typename T>
__global__ void __launch_bounds__(256) rnea_jvp_kernel(JvpArgs<T> G)
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
   const bool with_ext = A.fext != nullptr, with_dq = G.dq != nullptr, with_dqd = G.dqd != nullptr && A.coriolis != 0,
              with_dqdd = G.dqdd != nullptr, rhs = G.rhs != 0, with_in = rhs && G.tau_in != nullptr;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *qddrow = A.in3 + cfg * A.v_bs;
      const T *dqrow = G.dq + cfg * A.v_bs;
      const T *dqdrow = G.dqd + cfg * A.v_bs;
      const T *dqddrow = G.dqdd + cfg * A.v_bs;
      const T *frow = with_ext ? A.fext + cfg * A.f_bs : nullptr;
      const T *inrow = with_in ? G.tau_in + cfg * A.v_bs : nullptr;
      T *out = A.out + cfg * A.v_bs;
      // ---- outward sweep: velocity, acceleration and force of every body, and their tangents
      SV<T> v_prev = Z6, a_prev = Z6, xi_prev = Z6, dv_prev = Z6, da_prev = Z6;
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int s = slot[j];
         SV<T> vp, ap, xip, dvp, dap;
         if (parent < 0)
            vp = Z6, ap = root_acceleration(A), xip = Z6, dvp = Z6, dap = Z6;
         else if (flags & MF_PARENT_ADJ)
            vp = v_prev, ap = a_prev, xip = xi_prev, dvp = dv_prev, dap = da_prev;
         else
         {
            const int sp = slot[parent];
            vp = ws_load6(ws, ws_stride, sp + JS_V);
            ap = ws_load6(ws, ws_stride, sp + JS_A);
            xip = ws_load6(ws, ws_stride, sp + JS_XI);
            dvp = ws_load6(ws, ws_stride, sp + JS_DV);
            dap = ws_load6(ws, ws_stride, sp + JS_DA);
         }
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, s + JS_JP, true);
         const SV<T> vJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, A.coriolis != 0);
         const SV<T> aJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qddrow, A.v_es, A.accel != 0);
         const SV<T> Sq = joint_vec<T>(type, dof_map, mi[MI_DOF], dqrow, A.v_es, with_dq);
         const SV<T> Sv = joint_vec<T>(type, dof_map, mi[MI_DOF], dqdrow, A.v_es, with_dqd);
         const SV<T> Sa = joint_vec<T>(type, dof_map, mi[MI_DOF], dqddrow, A.v_es, with_dqdd);
         const SV<T> vl = motion_down(type, jx, Xb, vp), al = motion_down(type, jx, Xb, ap);
         const SV<T> v = vl + vJ;
         const SV<T> a = al + aJ + crm(v, vJ);
         const SV<T> xi = motion_down(type, jx, Xb, xip) + Sq;
         const SV<T> dv = motion_down(type, jx, Xb, dvp) + crm(vl, Sq) + Sv;
         const SV<T> da = motion_down(type, jx, Xb, dap) + crm(al, Sq) + Sa + crm(dv, vJ) + crm(v, Sv);
         const RI<T> I = load_inertia<T>(c);
         const SV<T> h = mul(I, v);
         SV<T> f = mul(I, a) + crf(v, h);
         SV<T> df = mul(I, da) + crf(dv, h) + crf(v, mul(I, dv));
         if (with_ext)
         {
            const SV<T> fe = load_fext<T>(c, frow, A.f_es, mi[MI_EXT]);
            f = f - fe;
            df = df + crf(xi, fe);
         }
         ws_store6(ws, ws_stride, s + JS_F, f);
         ws_store6(ws, ws_stride, s + JS_DF, df);
         if (flags & MF_STORE_VA)
         {
            ws_store6(ws, ws_stride, s + JS_V, v);
            ws_store6(ws, ws_stride, s + JS_A, a);
            ws_store6(ws, ws_stride, s + JS_XI, xi);
            ws_store6(ws, ws_stride, s + JS_DV, dv);
            ws_store6(ws, ws_stride, s + JS_DA, da);
         }
         v_prev = v, a_prev = a, xi_prev = xi, dv_prev = dv, da_prev = da;
      }
      // ---- inward sweep: the subtree's force and its tangent, and the entries of the body's DoFs
      SV<T> fcarry = Z6, dfcarry = Z6;
      bool have_carry = false;
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int s = slot[j];
         SV<T> F = ws_load6(ws, ws_stride, s + JS_F), dF = ws_load6(ws, ws_stride, s + JS_DF);
         if (have_carry)
            F = F + fcarry, dF = dF + dfcarry;
         have_carry = false;
         const int nd = dof_count(type);
         if (j % parts == part && nd > 0)
         {
            ciptr dj = dof_map + mi[MI_DOF];
            for (int k = 0; k < nd; k++)
            {
               const long at = (long)dj[k] * A.v_es;
               const T val = comp(dF, dof_comp(type, k));
               out[at] = rhs ? (with_in ? inrow[at] : T(0)) - val : val;
            }
         }
         // hand the force and its tangent to the parent: the step of this joint turns the force that goes up
         if (parent >= 0)
         {
            const XF<T> Xb = load_xb<T>(c);
            const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, s + JS_JP);
            const SV<T> Sq = joint_vec<T>(type, dof_map, mi[MI_DOF], dqrow, A.v_es, with_dq);
            const SV<T> Fu = force_up(type, jx, Xb, F), dFu = force_up(type, jx, Xb, dF + crf(Sq, F));
            if (flags & MF_PARENT_ADJ)
               fcarry = Fu, dfcarry = dFu, have_carry = true;
            else
            {
               const int sp = slot[parent];
               ws_add6(ws, ws_stride, sp + JS_F, Fu);
               ws_add6(ws, ws_stride, sp + JS_DF, dFu);
            }
         }
      }
      // entries no joint owns
      if (part == 0)
         for (int z = 0; z < G.n_unowned; z++)
            out[(long)unowned[z] * A.v_es] = T(0);
   }
}

} // namespace mh
