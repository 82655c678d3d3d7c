// mh_params_vjp_kernels.h -- reverse-mode gradient of the inverse dynamics with respect to the PER-CONFIGURATION inertial parameters: for a
// cotangent u of the efforts, u^T d tau / d pi of every configuration (run-time topology, one lane per configuration, gfx950).  pi and the
// gradient have the layout of mh_params_kernels.h: ten numbers per body, (mass, com, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz).
//
//   u^T tau = sum_d nu_d . f_d + (terms free of pi),    nu_d = sum_{a <= d} S_a u_a    (the nu of rnea_vjp_kernel: the motion of body d for
//                                                                                        qd = u; motion_down is the adjoint of force_up)
// and f_d = I_d a_d + v_d x* (I_d v_d), the Newton-Euler force rnea_parameters_kernel forms, is linear in the inertia record of body d and
// in nobody else's.  So there is one outward sweep and no inward one: the ten derivatives of body d are formed where nu_d, v_d and a_d are in
// registers, and stored once.  With nu . (v x* F) = -(v xm nu) . F,
//   nu . f = nu . (I a) + y . (I v),    y = -(v xm nu)
// two pairings y . (I x) of a motion pair with the inertia.  They are taken in the BODY-FIXED frame (nu, v, a carried there with the body's
// MC_RF / MC_PF, the inverse of the map inertia_from_parameters applies; pairings and cross products commute with the change of frame),
// where the record is (m, h = m c, J) of the ten numbers themselves: with I x = (J w + h x v, m v - h x w) for x = (w, v), y = (w_y, v_y)
//   d/dm = v_y . v      d/dh = v x w_y + v_y x w      d/dJ_aa = w_y,a w_a      d/dJ_ab = w_y,a w_b + w_y,b w_a  (one number for both entries)
// and the chain to (m, c, J) is  g_m = g^_m + c . g^_h,  g_c = m g^_h,  g_J = g^_J -- the only place pi is read.
// u = 0 gives exact zeros; a body outside the subtrees of the joints where u is not zero gets exact zeros (nu_d = 0).
//
// Storing the gradient: [10 n][B] (MH_LAYOUT_SOA) is one contiguous line per wave-instruction.  In [B][n][10] (MH_LAYOUT_AOS) the ten
// numbers of a lane would be ten stores with the lanes 10 n elements apart; a body's 64 x 10 block goes through the wave's staging buffer
// instead and leaves in the run pattern load_parameters reads pi with -- ten instructions, each over six or seven runs of 80 contiguous
// bytes --, the ragged last group included.
//
// gridDim.y waves may share a group of 64 configurations (small batches), as in rnea_vjp_kernel: each runs the sweep -- there is nothing
// else to run -- and forms and stores the blocks of every gridDim.y-th body.
//
// The block of a body (parameter_gradient) and its way out (store_parameters) are also what rnea_parameters_state_vjp_kernel
// (mh_params_state_vjp_kernels.h) calls from the outward sweep of the state gradients.
#pragma once
#include "mh_params_kernels.h"

namespace mh
{
template <typename T>
struct ParamVjpArgs
{
   ParamArgs<T> p; // a: m, B, q / qd / in3 = qdd and their strides, ws, root acceleration, the two RNEA switches (out, fext are not used); pi
   const T *u;     // [nv] cotangent of the efforts, strides of qd
   T *gpi;         // the gradient, laid out like pi (p_bs, p_es)
   int negate;     // store -gpi (the forward form: u = H^-1 w)
};

// the ten numbers g of body `ext` of this lane's configuration into gpi: load_parameters run backwards, with its lane index l.  Every lane
// of the wave that is still in the loop over the batch calls this together.
template <typename T>
MH_DEV void store_parameters(const ParamVjpArgs<T> &G, T *stage, int l, long first, long cfg, int ext, const T (&g)[PARAMS_PER_BODY])
{
   const long p_bs = G.p.p_bs, p_es = G.p.p_es;
   if (p_es != 1)
   { // lanes are neighbours in memory
      T *row = G.gpi + cfg * p_bs + (long)ext * PARAMS_PER_BODY * p_es;
#pragma unroll
      for (int k = 0; k < PARAMS_PER_BODY; k++)
         row[k * p_es] = g[k];
      return;
   }
   const long left = G.p.a.B - first;
   const int rows = left < 64 ? (int)left : 64; // lanes 0 .. rows - 1 are in the loop, the others have left it
   wave_lds_fence(); // every lane has taken what was staged before
#pragma unroll
   for (int k = 0; k < PARAMS_PER_BODY; k++)
      stage[k * PARAMS_STAGE_PITCH + l] = g[k];
   wave_lds_fence();
#pragma unroll
   for (int i = 0; i < PARAMS_PER_BODY; i++)
   {
      const int idx = l + rows * i, r = idx / PARAMS_PER_BODY, k = idx - PARAMS_PER_BODY * r;
      G.gpi[(first + r) * p_bs + (long)ext * PARAMS_PER_BODY + k] = stage[k * PARAMS_STAGE_PITCH + r];
   }
}

// d (y . I x) / d (m, h, J) added to g^ = (m, h_x, h_y, h_z, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz)
template <typename T>
MH_DEV void pairing_gradient(const SV<T> &y, const SV<T> &x, T (&g)[PARAMS_PER_BODY])
{
   const V3<T> gh = cross(x.l, y.a) + cross(y.l, x.a);
   g[0] += dot(y.l, x.l);
   g[1] += gh.x, g[2] += gh.y, g[3] += gh.z;
   g[4] += y.a.x * x.a.x;
   g[5] += y.a.x * x.a.y + y.a.y * x.a.x;
   g[6] += y.a.x * x.a.z + y.a.z * x.a.x;
   g[7] += y.a.y * x.a.y;
   g[8] += y.a.y * x.a.z + y.a.z * x.a.y;
   g[9] += y.a.z * x.a.z;
}

// the parameter block of a body: g = sign * d (nu . f) / d (m, c, J) from the body's (nu, v, a) in its canonical frame, its constants c
// (MC_RF, MC_PF) and its ten numbers par.  rnea_parameters_vjp_kernel and rnea_parameters_state_vjp_kernel both form it here.
template <typename T, class CR>
MH_DEV void parameter_gradient(const CR &c, const SV<T> &nu, const SV<T> &v, const SV<T> &a, const T (&par)[PARAMS_PER_BODY], T sign,
                               T (&g)[PARAMS_PER_BODY])
{
   XF<T> Xf;
   Xf.R = M3<T>{c[MC_RF + 0], c[MC_RF + 1], c[MC_RF + 2], c[MC_RF + 3], c[MC_RF + 4], c[MC_RF + 5], c[MC_RF + 6], c[MC_RF + 7], c[MC_RF + 8]};
   Xf.p = V3<T>{c[MC_PF + 0], c[MC_PF + 1], c[MC_PF + 2]};
   const SV<T> nb = motion_to_child(Xf, nu), vb = motion_to_child(Xf, v), ab = motion_to_child(Xf, a);
   const SV<T> y = crm(nb, vb); // = -(v xm nu)
   T gh[PARAMS_PER_BODY] = {T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)};
   pairing_gradient(nb, ab, gh);
   pairing_gradient(y, vb, gh);
   g[0] = sign * (gh[0] + (par[1] * gh[1] + par[2] * gh[2] + par[3] * gh[3]));
   const T sm = sign * par[0];
   g[1] = sm * gh[1], g[2] = sm * gh[2], g[3] = sm * gh[3];
#pragma unroll
   for (int k = 4; k < PARAMS_PER_BODY; k++)
      g[k] = sign * gh[k];
}

template <typename T>
__global__ void __launch_bounds__(256) rnea_parameters_vjp_kernel(ParamVjpArgs<T> G)
{
   __shared__ T stage[PARAMS_PER_BODY * PARAMS_STAGE_PITCH];
   const Args<T> &A = G.p.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)m.n_slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};
   const SV<T> Z6{Z, Z};
   const T sign = G.negate ? T(-1) : T(1);

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const long first = cfg - (lane & 63);
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *qddrow = A.in3 + cfg * A.v_bs;
      const T *urow = G.u + cfg * A.v_bs;
      // ---- the outward sweep of rnea_parameters_kernel, nu beside v and a.  A body whose children do not all directly follow it parks
      //      (v, a) in its MI_SLOT_VA and nu in its MI_SLOT_F, which holds no force here.
      SV<T> v_prev = Z6, a_prev = Z6, nu_prev = Z6;
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         SV<T> vp, ap, nup;
         if (parent < 0)
            vp = Z6, ap = root_acceleration(A), nup = Z6;
         else if (flags & MF_PARENT_ADJ)
            vp = v_prev, ap = a_prev, nup = nu_prev;
         else
         {
            ciptr pmi = meta + parent * MI_STRIDE;
            vp = ws_load6(ws, ws_stride, pmi[MI_SLOT_VA]);
            ap = ws_load6(ws, ws_stride, pmi[MI_SLOT_VA] + 6);
            nup = ws_load6(ws, ws_stride, pmi[MI_SLOT_F]);
         }
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP], false);
         const SV<T> vJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, A.coriolis != 0);
         const SV<T> aJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qddrow, A.v_es, A.accel != 0);
         const SV<T> Su = joint_vec<T>(type, dof_map, mi[MI_DOF], urow, A.v_es, true);
         SV<T> v = motion_down(type, jx, Xb, vp) + vJ;
         const SV<T> a = motion_down(type, jx, Xb, ap) + aJ + crm(v, vJ);
         const SV<T> nu = motion_down(type, jx, Xb, nup) + Su;
         if (!A.coriolis)
            v = Z6;
         if (flags & MF_STORE_VA)
         {
            ws_store6(ws, ws_stride, mi[MI_SLOT_VA], v);
            ws_store6(ws, ws_stride, mi[MI_SLOT_VA] + 6, a);
            ws_store6(ws, ws_stride, mi[MI_SLOT_F], nu);
         }
         v_prev = v, a_prev = a, nu_prev = nu;
         if (j % parts != part)
            continue;
         // ---- the block of this body
         T par[PARAMS_PER_BODY], g[PARAMS_PER_BODY];
         load_parameters(G.p, stage, threadIdx.x & 63, first, cfg, mi[MI_EXT], par);
         parameter_gradient<T>(c, nu, v, a, par, sign, g);
         store_parameters(G, stage, threadIdx.x & 63, first, cfg, mi[MI_EXT], g);
      }
   }
}

} // namespace mh
