// mh_params_state_vjp_kernels.h -- reverse-mode gradients of the inverse dynamics at PER-CONFIGURATION inertial parameters, with respect
// to the state AND the parameters in one pair of sweeps: for a cotangent u of the efforts of rnea_parameters_kernel, u^T d tau / d q,
// u^T d tau / d qd, H(pi) u and u^T d tau / d pi of every configuration (run-time topology, one lane per configuration, gfx950).
//
// The state gradients are those of rnea_vjp_kernel (mh_rnea_vjp_kernels.h, whose notation, workspace slots and formulas this file keeps)
// with the rigid inertia of a body taken from the lane's ten numbers (the read of load_parameters, inertia_from_parameters of
// mh_params_kernels.h) where that kernel calls load_inertia.  The parameter gradient is that of rnea_parameters_vjp_kernel
// (mh_params_vjp_kernels.h): the two pairings nu . (I a) + y . (I v) in the body-fixed frame and the chain to (m, c, J).  That kernel
// runs an outward sweep of its own only to have (nu, v, a) of a body in registers; the outward sweep of the state gradients has all
// three, so the ten derivatives are formed there, after the body's force and motions are parked -- nothing of them is live while the
// block is formed and leaves.  The block (parameter_gradient) and the staged read and store of the ten numbers (load_parameters,
// store_parameters, here with staging_lane() for the lane index) are the functions of mh_params_vjp_kernels.h and mh_params_kernels.h.
// The two sweeps are a COPY of rnea_vjp_kernel's, kept in step by hand: written once as function templates over the inertia's source
// they compiled to other register counts and, by other fused multiply-adds, to other last bits -- a change to
// a sweep there is made here too.
//
// The inertia is needed in both sweeps (I a + v x* I v going out, Ic and the factorised inertia coming in).  It is formed twice from pi,
// as aba_parameters_kernel forms it, and not parked: parking costs ten stores and ten loads per body and a slot plan of its own; reading
// pi again costs the ten loads and about 60 flops, and the slot plan stays rnea_vjp_kernel's (vjp_slot_plan).  The staged AoS read is a
// wave-wide operation: both sweeps are loops over the bodies with wave-uniform bounds and no lane leaves them early, so every lane still
// in the batch loop reaches the staged read of a body together, whichever bodies its wave owns.
//
// gridDim.y waves may share a group of 64 configurations (small batches), as in rnea_vjp_kernel: each runs both sweeps; the wave with
// j % parts == part stores the entries of body j's DoFs and body j's ten parameter derivatives.  Every output entry is written once, no
// atomics, no memset.  u = 0 gives exact zeros in every output, consider_coriolis = 0 exact zeros in gqd.
#pragma once
#include "mh_params_vjp_kernels.h"
#include "mh_rnea_vjp_kernels.h"

namespace mh
{
template <typename T>
struct ParamStateVjpArgs
{
   ParamVjpArgs<T> pv;  // p.a: m, B, q, qd, in3 = qdd, fext (or NULL), ws, root acceleration, the switches (out is not used); p.pi;
                        // u; gpi (or NULL); negate: store -gq, -gqd and -gpi (the forward form: u = H^-1 w)
   T *gq, *gqd, *gqdd;  // [nv] each, strides of qd; any may be NULL
   const int *slot;     // [n] first workspace slot of every body (vjp_slot_plan)
   int slots;           // workspace slots per lane
   const int *unowned;  // DoF indices no joint owns: zeros
   int n_unowned;
};

template <typename T>
__global__ void __launch_bounds__(256) rnea_parameters_state_vjp_kernel(ParamStateVjpArgs<T> G)
{
   __shared__ T stage[PARAMS_PER_BODY * PARAMS_STAGE_PITCH];
   const Args<T> &A = G.pv.p.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const ciptr slot = as_const(G.slot), unowned = as_const(G.unowned);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)G.slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};
   const SV<T> Z6{Z, Z};
   const bool with_ext = A.fext != nullptr, with_gq = G.gq != nullptr, with_gqd = G.gqd != nullptr, with_gqdd = G.gqdd != nullptr;
   const bool with_gpi = G.pv.gpi != nullptr, with_state = with_gq || with_gqd || with_gqdd;
   const T sign = G.pv.negate ? T(-1) : T(1);

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      // the configuration of the wave's lane 0 (= cfg - (lane & 63): a workgroup is one wave, plan_launch, and lane 0 is the last to
      // leave the loop), read as a scalar and not kept per lane
      const long first = ((long)__builtin_amdgcn_readfirstlane((int)(cfg >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)cfg);
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *qddrow = A.in3 + cfg * A.v_bs;
      const T *urow = G.pv.u + cfg * A.v_bs;
      const T *frow = with_ext ? A.fext + cfg * A.f_bs : nullptr;
      T *gq = with_gq ? G.gq + cfg * A.v_bs : nullptr;
      T *gqd = with_gqd ? G.gqd + cfg * A.v_bs : nullptr;
      T *gqdd = with_gqdd ? G.gqdd + cfg * A.v_bs : nullptr;
      // ---- outward sweep: velocities, accelerations, the Newton-Euler force and the momentum of every body; nu beside them; the
      //      parameter derivatives of the bodies this wave owns
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
         // (read here and not at the top of the body: the ten numbers are not live across the kinematics)
         T par[PARAMS_PER_BODY];
         load_parameters(G.pv.p, stage, staging_lane(), first, cfg, mi[MI_EXT], par);
         if (with_state)
         {
            const RI<T> I = inertia_from_parameters<T>(c, par);
            const SV<T> h = mul(I, v);
            SV<T> f = mul(I, a) + crf(v, h);
            if (with_ext)
            {
               const SV<T> fe = load_fext<T>(c, frow, A.f_es, mi[MI_EXT]);
               f = f - fe;
               ws_store6(ws, ws_stride, s + VS_W, fe);
            }
            ws_store6(ws, ws_stride, s + VS_F, f);
            ws_store6(ws, ws_stride, s + VS_H, h);
            ws_store6(ws, ws_stride, s + VS_VL, vl);
            ws_store6(ws, ws_stride, s + VS_AL, al);
            ws_store6(ws, ws_stride, s + VS_NUL, nul);
         }
         ws_store6(ws, ws_stride, s + VS_V, v);
         if (flags & MF_STORE_VA)
         {
            ws_store6(ws, ws_stride, s + VS_A, a);
            ws_store6(ws, ws_stride, s + VS_NU, nu);
            ws_store6(ws, ws_stride, s + VS_T1, Z6);
            ws_store6(ws, ws_stride, s + VS_T4, Z6);
            ws_store6(ws, ws_stride, s + VS_T5, Z6);
         }
         v_prev = v, a_prev = a, nu_prev = nu;
         // ---- the parameter block of this body (parameter_gradient of mh_params_vjp_kernels.h, as in rnea_parameters_vjp_kernel);
         //      store_parameters is wave-wide like load_parameters, and the condition is the wave's
         if (with_gpi && j % parts == part)
         {
            T g[PARAMS_PER_BODY];
            parameter_gradient<T>(c, nu, v, a, par, sign, g);
            store_parameters(G.pv, stage, staging_lane(), first, cfg, mi[MI_EXT], g);
         }
      }
      if (!with_state) // (wave-uniform: the inward sweep has nothing to store)
         continue;
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
         T par[PARAMS_PER_BODY];
         load_parameters(G.pv.p, stage, staging_lane(), first, cfg, mi[MI_EXT], par);
         const SV<T> vj = ws_load6(ws, ws_stride, s + VS_V);
         RI<T> Ic = inertia_from_parameters<T>(c, par);
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
                     gqd[(long)dj[k] * A.v_es] = sign * comp(Gv, dof_comp(type, k));
               }
               if (with_gq)
               {
                  const SV<T> al = ws_load6(ws, ws_stride, s + VS_AL);
                  SV<T> X5 = T5 - crf(nul, F);
                  if (with_ext)
                     X5 = X5 - crf(nu, W);
                  const SV<T> Gq = X5 - crf(vl, X4 - crf(vl, X1)) - crf(al, X1);
                  for (int k = 0; k < nd; k++)
                     gq[(long)dj[k] * A.v_es] = sign * comp(Gq, dof_comp(type, k));
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
                  RI<T> racc = ws_load_ri(ws, ws_stride, sp + VS_IC);
                  add(racc, Ic);
                  ws_store_ri(ws, ws_stride, sp + VS_IC, racc);
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
      if (part == 0)
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
