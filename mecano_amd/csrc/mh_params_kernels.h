// mh_params_kernels.h -- inverse and forward dynamics with PER-CONFIGURATION inertial parameters (run-time topology, one lane per
// configuration, gfx950).
//
// rnea_kernel / aba_kernel of mh_kernels.h evaluate B states of ONE robot: the rigid inertia of a body is the model's constant
// (load_inertia: MC_M, MC_H, MC_I).  Here every configuration brings the ten inertial numbers of every body,
//   (mass, com_x, com_y, com_z, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz)      -- mh_model_desc's inertia_mass, inertia_com and the symmetric part of
//                                                                     inertia_J: J about the origin of the body-fixed frame, in its axes
// for joint j in mh_model_desc order at elements [10 j, 10 j + 10) of its row of pi (the order of mh_regressor_* and of
// OracleModel.parameter_vector).  Topology, joint frames, axes and index maps stay the model's.  A lane turns the ten numbers of a body
// into the canonical record (m, h, I about the canonical after-joint origin) with the body's constant MC_RF / MC_PF -- the map
// mh_model_create applies once on the host, about 60 flops -- in registers, where the fixed-parameter kernels call load_inertia.
// Forward dynamics needs the record in pass one (bias wrench) and in pass two (articulated inertia): it is formed twice rather than
// parked in the workspace, which would cost ten stores and ten loads per body to save the 60 flops.
//
// Reading pi: [10 n][B] (MH_LAYOUT_SOA) is one contiguous line per wave-instruction, like every workspace access.  In [B][n][10]
// (MH_LAYOUT_AOS) neighbouring lanes are 10 n elements apart; the lanes of a wave read a body's 64 x 10 block together instead -- 640
// elements in ten instructions, each over six or seven runs of 80 contiguous bytes -- into LDS (5 KB in fp64), and every lane takes its
// ten from there.  In the ragged last group the lanes still in the loop share the rows that exist.  One wave per workgroup
// (plan_launch): the staging buffer is the wave's own and needs no workgroup barrier, only the ordering of the wave's LDS traffic.
// (Keeping all 64 lanes in the loop, a lane beyond the batch redoing the last row without storing, cost aba_parameters_kernel<double>
// 64 bytes of scratch per lane; with the loop of the fixed-parameter kernels it has none.)
//
// The sweeps are those of rnea_kernel and aba_kernel (effort-source joints only, no per-body outputs), statement for statement apart
// from the inertia; they are copies and not templates over the inertia's source because mh_kernels.h is hashed into every code object
// and its kernels' results are pinned bit for bit (as mh_minv_kernels.h copies the articulated-inertia phase).
#pragma once
#include "mh_kernels.h"

namespace mh
{
#define MH_WS(slot) ws[(long)(slot)*ws_stride]

constexpr int PARAMS_PER_BODY = 10;
constexpr int PARAMS_STAGE_PITCH = 65; // rows of the staging buffer: 64 lanes + 1, so that the ten writes of a lane fall into different banks

template <typename T>
struct ParamArgs
{
   Args<T> a;       // m, B, q / qd / in3 / fext and their strides, out, ws, root acceleration, the two RNEA switches
   const T *pi;     // inertial parameters of every configuration
   long p_bs, p_es; // batch / element strides of pi (element = 10 * joint in mh_model_desc order + k)
};

// the canonical record of a body from its ten numbers: the inertia in the body-fixed frame, handed through (MC_RF, MC_PF) like a rigid
// inertia through a fixed transform (mh_api.hip, mh_model_create: "spatial inertia about the canonical after-joint origin")
template <typename T, class CR>
MH_DEV RI<T> inertia_from_parameters(const CR &c, const T (&p)[PARAMS_PER_BODY])
{
   const M3<T> Rf{c[MC_RF + 0], c[MC_RF + 1], c[MC_RF + 2], c[MC_RF + 3], c[MC_RF + 4], c[MC_RF + 5], c[MC_RF + 6], c[MC_RF + 7], c[MC_RF + 8]};
   const V3<T> pf{c[MC_PF + 0], c[MC_PF + 1], c[MC_PF + 2]};
   RI<T> r;
   r.m = p[0];
   r.h = mul(Rf, V3<T>{p[0] * p[1], p[0] * p[2], p[0] * p[3]});
   r.I = conj(Rf, S3<T>{p[4], p[5], p[6], p[7], p[8], p[9]});
   shift_origin(r, pf);
   return r;
}

// Orders the LDS traffic of ONE wave: its LDS instructions complete in the order they were issued, so all that is needed is that the
// compiler neither moves an access across this point nor keeps a staged value in a register.  (A workgroup of these kernels is one wave.)
MH_DEV void wave_lds_fence()
{
   asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The lane index for load_parameters / store_parameters, formed anew at every call.  With threadIdx.x & 63 passed in, the ten (row, number)
// pairs of a lane and the addresses made of them do not depend on the body, so the compiler keeps them in registers across the sweeps:
// about 50 in rnea_parameters_state_vjp_kernel, which has none to spare (fp32: 266 registers and one wave per SIMD with them, against 211
// and two for rnea_vjp_kernel).  An empty asm on the lane index makes them a dozen integer operations per body instead.
MH_DEV int staging_lane()
{
   int l = threadIdx.x & 63;
   asm volatile("" : "+v"(l));
   return l;
}

// the ten numbers of body `ext` (mh_model_desc order) of this lane's configuration.  l = the lane's index in its wave (threadIdx.x & 63,
// or staging_lane()), first = configuration of the wave's lane 0, cfg = this lane's; every lane of the wave that is still in the loop
// over the batch calls this together.
template <typename T>
MH_DEV void load_parameters(const ParamArgs<T> &G, T *stage, int l, long first, long cfg, int ext, T (&p)[PARAMS_PER_BODY])
{
   if (G.p_es != 1)
   { // lanes are neighbours in memory
      const T *row = G.pi + cfg * G.p_bs + (long)ext * PARAMS_PER_BODY * G.p_es;
#pragma unroll
      for (int k = 0; k < PARAMS_PER_BODY; k++)
         p[k] = row[k * G.p_es];
      return;
   }
   const long left = G.a.B - first;
   const int rows = left < 64 ? (int)left : 64; // lanes 0 .. rows - 1 are in the loop, the others have left it
   wave_lds_fence(); // every lane has taken the previous body's numbers
#pragma unroll
   for (int i = 0; i < PARAMS_PER_BODY; i++)
   {
      const int idx = l + rows * i, r = idx / PARAMS_PER_BODY, k = idx - PARAMS_PER_BODY * r;
      stage[k * PARAMS_STAGE_PITCH + r] = G.pi[(first + r) * G.p_bs + (long)ext * PARAMS_PER_BODY + k];
   }
   wave_lds_fence();
#pragma unroll
   for (int k = 0; k < PARAMS_PER_BODY; k++)
      p[k] = stage[k * PARAMS_STAGE_PITCH + l];
}

// ============================================================================================ inverse dynamics
// rnea_kernel<T, false> with the body's inertia from the lane's parameters (InverseDynamicsCalculator.java:873-959)
template <typename T>
__global__ void __launch_bounds__(256) rnea_parameters_kernel(ParamArgs<T> G)
{
   __shared__ T stage[PARAMS_PER_BODY * PARAMS_STAGE_PITCH];
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   T *ws = A.ws + (lane >> 6) * ((long)m.n_slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const long first = cfg - (lane & 63);
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *qddrow = A.in3 + cfg * A.v_bs;
      const T *frow = A.fext ? A.fext + cfg * A.f_bs : nullptr;
      T *trow = A.out + cfg * A.v_bs;

      // ---- outward sweep: velocities, accelerations, Newton-Euler wrench of every body
      SV<T> v_prev{Z, Z}, a_prev{Z, Z};
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         T par[PARAMS_PER_BODY];
         load_parameters(G, stage, threadIdx.x & 63, first, cfg, mi[MI_EXT], par);
         SV<T> vp, ap;
         if (parent < 0)
         {
            vp = SV<T>{Z, Z};
            ap = root_acceleration(A);
         }
         else if (flags & MF_PARENT_ADJ)
         {
            vp = v_prev, ap = a_prev;
         }
         else
         {
            const int sp = meta[parent * MI_STRIDE + MI_SLOT_VA];
            vp = ws_load6(ws, ws_stride, sp);
            ap = ws_load6(ws, ws_stride, sp + 6);
         }
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP], true);
         const SV<T> vJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, A.coriolis != 0);
         const SV<T> aJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qddrow, A.v_es, A.accel != 0);
         SV<T> v = motion_down(type, jx, Xb, vp) + vJ;
         SV<T> a = motion_down(type, jx, Xb, ap) + aJ + crm(v, vJ);
         if (!A.coriolis)
            v = SV<T>{Z, Z};
         const RI<T> I = inertia_from_parameters<T>(c, par);
         SV<T> f = mul(I, a) + crf(v, mul(I, v));
         if (frow)
            f = f - load_fext<T>(c, frow, A.f_es, mi[MI_EXT]);
         ws_store6(ws, ws_stride, mi[MI_SLOT_F], f);
         if (flags & MF_STORE_VA)
         {
            ws_store6(ws, ws_stride, mi[MI_SLOT_VA], v);
            ws_store6(ws, ws_stride, mi[MI_SLOT_VA] + 6, a);
         }
         v_prev = v, a_prev = a;
      }
      // ---- inward sweep: joint efforts, wrenches handed to the parents
      SV<T> carry{Z, Z};
      bool have_carry = false;
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         SV<T> f = ws_load6(ws, ws_stride, mi[MI_SLOT_F]);
         if (have_carry)
            f = f + carry;
         ciptr di = dof_map + mi[MI_DOF];
         if (type == JT_REVOLUTE)
            trow[di[0] * A.v_es] = f.a.z;
         else if (type == JT_PRISMATIC)
            trow[di[0] * A.v_es] = f.l.z;
         else if (type == JT_SIXDOF)
         {
            trow[di[0] * A.v_es] = f.a.x, trow[di[1] * A.v_es] = f.a.y, trow[di[2] * A.v_es] = f.a.z;
            trow[di[3] * A.v_es] = f.l.x, trow[di[4] * A.v_es] = f.l.y, trow[di[5] * A.v_es] = f.l.z;
         }
         else if (type == JT_PLANAR || type == JT_SPHERICAL)
         {
            const V3<T> t3 = comp3(type, f);
            trow[di[0] * A.v_es] = t3.x, trow[di[1] * A.v_es] = t3.y, trow[di[2] * A.v_es] = t3.z;
         }
         have_carry = false;
         if (parent >= 0)
         {
            const XF<T> Xb = load_xb<T>(c);
            const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
            const SV<T> fp = force_up(type, jx, Xb, f);
            if (flags & MF_PARENT_ADJ)
            {
               carry = fp;
               have_carry = true;
            }
            else
               ws_add6(ws, ws_stride, meta[parent * MI_STRIDE + MI_SLOT_F], fp);
         }
      }
   }
}

// ============================================================================================ forward dynamics
// aba_kernel<T, false, false> with the body's inertia from the lane's parameters (ForwardDynamicsCalculator.java:1085-1310)
template <typename T>
__global__ void __launch_bounds__(256) aba_parameters_kernel(ParamArgs<T> G)
{
   __shared__ T stage[PARAMS_PER_BODY * PARAMS_STAGE_PITCH];
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64;
   T *ws = A.ws + (lane >> 6) * ((long)m.n_slots * 64) + (lane & 63);
   const V3<T> Z{T(0), T(0), T(0)};

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const long first = cfg - (lane & 63);
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *taurow = A.in3 + cfg * A.v_bs;
      const T *frow = A.fext ? A.fext + cfg * A.f_bs : nullptr;
      T *orow = A.out + cfg * A.v_bs;

      // ---- pass one (:1085-1127): velocities, bias wrench p, bias acceleration c
      SV<T> v_prev{Z, Z};
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type_rt = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         T par[PARAMS_PER_BODY];
         load_parameters(G, stage, threadIdx.x & 63, first, cfg, mi[MI_EXT], par);
         auto body = [&](auto kind) { // one dispatch on the joint kind per body, straight-line code per kind (as in aba_kernel)
            const int type = kind;
            SV<T> vp;
            if (parent < 0)
               vp = SV<T>{Z, Z};
            else if (flags & MF_PARENT_ADJ)
               vp = v_prev;
            else
               vp = ws_load6(ws, ws_stride, meta[parent * MI_STRIDE + MI_SLOT_VA]);
            const XF<T> Xb = load_xb<T>(c);
            JX<T> jx;
            SV<T> vJ{Z, Z};
            if (type == JT_REVOLUTE)
            {
               jx.d = T(0);
               sincos_t(qrow[mi[MI_ROW_Q] * A.q_es], jx.s, jx.c);
               MH_WS(mi[MI_SLOT_JP]) = jx.c, MH_WS(mi[MI_SLOT_JP] + 1) = jx.s;
               vJ.a.z = qdrow[mi[MI_ROW_V] * A.v_es];
            }
            else if (type == JT_PRISMATIC)
               jx.c = T(1), jx.s = T(0), jx.d = qrow[mi[MI_ROW_Q] * A.q_es], vJ.l.z = qdrow[mi[MI_ROW_V] * A.v_es];
            else
            {
               jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP], true);
               vJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, true);
            }
            const SV<T> v = motion_down(type, jx, Xb, vp) + vJ;
            const RI<T> I = inertia_from_parameters<T>(c, par);
            SV<T> p = crf(v, mul(I, v));
            if (frow)
               p = p - load_fext<T>(c, frow, A.f_es, mi[MI_EXT]);
            ws_store6(ws, ws_stride, mi[MI_SLOT_F], p);
            ws_store6(ws, ws_stride, mi[MI_SLOT_C], crm(v, vJ));
            if (flags & MF_STORE_VA)
               ws_store6(ws, ws_stride, mi[MI_SLOT_VA], v);
            v_prev = v;
         };
         switch (type_rt)
         {
            case JT_REVOLUTE: body(std::integral_constant<int, JT_REVOLUTE>{}); break;
            case JT_PRISMATIC: body(std::integral_constant<int, JT_PRISMATIC>{}); break;
            case JT_SIXDOF: body(std::integral_constant<int, JT_SIXDOF>{}); break;
            case JT_PLANAR: body(std::integral_constant<int, JT_PLANAR>{}); break;
            case JT_SPHERICAL: body(std::integral_constant<int, JT_SPHERICAL>{}); break;
            default: body(std::integral_constant<int, JT_FIXED>{}); break;
         }
      }
      // ---- pass two (:1136-1254): articulated inertias and bias wrenches, leaves to root
      ABI<T> Icarry;
      SV<T> pcarry{Z, Z};
      bool have_carry = false;
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type_rt = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         T par[PARAMS_PER_BODY];
         load_parameters(G, stage, threadIdx.x & 63, first, cfg, mi[MI_EXT], par);
         auto body = [&](auto kind) {
            const int type = kind;
            ABI<T> IA = abi_from_rigid(inertia_from_parameters<T>(c, par));
            SV<T> pA = ws_load6(ws, ws_stride, mi[MI_SLOT_F]);
            if (have_carry)
            {
               add(IA, Icarry);
               pA = pA + pcarry;
            }
            if (flags & MF_HAS_ACC)
               add(IA, ws_load_abi(ws, ws_stride, mi[MI_SLOT_IA]));
            have_carry = false;
            const int sf = mi[MI_SLOT_F];
            ciptr di = dof_map + mi[MI_DOF];
            ABI<T> Ia = IA;
            SV<T> pa = pA;
            bool handed_up = false;
            if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            {
               V3<T> ua, ul;
               T D, pz;
               if (type == JT_REVOLUTE)
               {
                  ua = V3<T>{IA.A.xz, IA.A.yz, IA.A.zz}, ul = V3<T>{IA.C.zx, IA.C.zy, IA.C.zz};
                  D = IA.A.zz, pz = pA.a.z;
               }
               else
               {
                  ua = V3<T>{IA.C.xz, IA.C.yz, IA.C.zz}, ul = V3<T>{IA.L.xz, IA.L.yz, IA.L.zz};
                  D = IA.L.zz, pz = pA.l.z;
               }
               const T dinv = T(1) / D;                                  // :1183 (unguarded, as the reference's)
               const T u = taurow[mi[MI_ROW_V] * A.v_es] - pz;           // :1200-1215
               ws_store6(ws, ws_stride, sf, SV<T>{ua, ul});
               MH_WS(sf + 6) = dinv;
               MH_WS(sf + 7) = u;
               if (parent >= 0)
               {
                  const SV<T> cj = ws_load6(ws, ws_stride, mi[MI_SLOT_C]);
                  const T ud = u * dinv;
                  if (type == JT_REVOLUTE)
                  {
                     rank1_down_revolute(Ia, ua, ul, dinv);              // :1220-1226
                     pa = pA + mul(Ia, cj) + SV<T>{ud * ua, ud * ul};    // :1229-1234
                     JX<T> jx;
                     jx.c = MH_WS(mi[MI_SLOT_JP]), jx.s = MH_WS(mi[MI_SLOT_JP] + 1), jx.d = T(0);
                     revolute_up(jx, load_xb<T>(c), Ia, pa);             // :1156-1166; pa is now expressed in the parent's frame
                     handed_up = true;
                  }
                  else
                  {
                     rank1_down(Ia, ua, ul, dinv);
                     pa = pA + mul(Ia, cj) + SV<T>{ud * ua, ud * ul};
                  }
               }
            }
            else if (type == JT_PLANAR || type == JT_SPHERICAL)
            { // 3-DoF joint: U = IA S (6 x 3), D = S^T U (3 x 3), u = tau - S^T pA   (:1177-1215 with N = 3)
               const SV<T> U0 = mul(IA, unit_twist<T>(type, 0)), U1 = mul(IA, unit_twist<T>(type, 1)), U2 = mul(IA, unit_twist<T>(type, 2));
               const V3<T> d0 = comp3(type, U0), d1 = comp3(type, U1), d2 = comp3(type, U2);
               const S3<T> Di = spd3_inverse(S3<T>{d0.x, d0.y, d0.z, d1.y, d1.z, d2.z});
               const V3<T> tau3{taurow[di[0] * A.v_es], taurow[di[1] * A.v_es], taurow[di[2] * A.v_es]};
               const V3<T> u3 = tau3 - comp3(type, pA);
               const int sl = mi[MI_SLOT_LK];
               ws_store6(ws, ws_stride, sl, U0), ws_store6(ws, ws_stride, sl + 6, U1), ws_store6(ws, ws_stride, sl + 12, U2);
               MH_WS(sl + 18) = Di.xx, MH_WS(sl + 19) = Di.xy, MH_WS(sl + 20) = Di.xz, MH_WS(sl + 21) = Di.yy, MH_WS(sl + 22) = Di.yz, MH_WS(sl + 23) = Di.zz;
               MH_WS(sl + 24) = u3.x, MH_WS(sl + 25) = u3.y, MH_WS(sl + 26) = u3.z;
               if (parent >= 0)
               { // Ia = IA - U D^-1 U^T ; pa = pA + Ia c + U D^-1 u   (:1220-1234)
                  const SV<T> W0 = Di.xx * U0 + Di.xy * U1 + Di.xz * U2, W1 = Di.xy * U0 + Di.yy * U1 + Di.yz * U2, W2 = Di.xz * U0 + Di.yz * U1 + Di.zz * U2;
                  rank1_pair_down(Ia, W0, U0), rank1_pair_down(Ia, W1, U1), rank1_pair_down(Ia, W2, U2);
                  const SV<T> cj = ws_load6(ws, ws_stride, mi[MI_SLOT_C]);
                  pa = pA + mul(Ia, cj) + u3.x * W0 + u3.y * W1 + u3.z * W2;
               }
            }
            else if (type == JT_SIXDOF)
            { // S = 1_6: U = IA, D = IA.  Pass three needs only x = IA^-1 u; for the parent Ia = 0 and pa = pA + u = tau.
               const SV<T> tau{V3<T>{taurow[di[0] * A.v_es], taurow[di[1] * A.v_es], taurow[di[2] * A.v_es]},
                               V3<T>{taurow[di[3] * A.v_es], taurow[di[4] * A.v_es], taurow[di[5] * A.v_es]}};
               const SV<T> x = spd6_solve(IA, tau - pA);
               ws_store6(ws, ws_stride, sf, x);
               if (parent >= 0)
               {
                  Ia.A = S3<T>{T(0), T(0), T(0), T(0), T(0), T(0)};
                  Ia.L = Ia.A;
                  Ia.C = M3<T>{T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)};
                  pa = tau;
               }
            }
            else if (parent >= 0)
            { // fixed joint: the whole articulated body is handed over unchanged (c = 0)
               pa = pA;
            }
            if (parent >= 0)
            {
               SV<T> pp = pa;
               if (!handed_up)
               {
                  const XF<T> Xb = load_xb<T>(c);
                  const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
                  if (type == JT_REVOLUTE)
                     revolute_up(jx, Xb, Ia, pp);
                  else
                  {
                     if (type != JT_SIXDOF) // an effort-source floating joint transmits no inertia: Ia = 0 stays 0
                        abi_up(type, jx, Xb, Ia); // :1156-1166
                     pp = force_up(type, jx, Xb, pa);
                  }
               }
               if (flags & MF_PARENT_ADJ)
               {
                  Icarry = Ia, pcarry = pp, have_carry = true;
               }
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
                  ws_add6(ws, ws_stride, pmi[MI_SLOT_F], pp);
               }
            }
         };
         switch (type_rt)
         {
            case JT_REVOLUTE: body(std::integral_constant<int, JT_REVOLUTE>{}); break;
            case JT_PRISMATIC: body(std::integral_constant<int, JT_PRISMATIC>{}); break;
            case JT_SIXDOF: body(std::integral_constant<int, JT_SIXDOF>{}); break;
            case JT_PLANAR: body(std::integral_constant<int, JT_PLANAR>{}); break;
            case JT_SPHERICAL: body(std::integral_constant<int, JT_SPHERICAL>{}); break;
            default: body(std::integral_constant<int, JT_FIXED>{}); break;
         }
      }
      // ---- pass three (:1259-1310): joint accelerations, root to leaves
      SV<T> a_prev{Z, Z};
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type_rt = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         auto body = [&](auto kind) {
            const int type = kind;
            SV<T> ap;
            if (parent < 0)
               ap = root_acceleration(A); // :259-264
            else if (flags & MF_PARENT_ADJ)
               ap = a_prev;
            else
               ap = ws_load6(ws, ws_stride, meta[parent * MI_STRIDE + MI_SLOT_VA]);
            const XF<T> Xb = load_xb<T>(c);
            JX<T> jx;
            if (type == JT_REVOLUTE)
               jx.c = MH_WS(mi[MI_SLOT_JP]), jx.s = MH_WS(mi[MI_SLOT_JP] + 1), jx.d = T(0);
            else if (type == JT_PRISMATIC)
               jx.c = T(1), jx.s = T(0), jx.d = qrow[mi[MI_ROW_Q] * A.q_es];
            else
               jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
            SV<T> a = motion_down(type, jx, Xb, ap) + ws_load6(ws, ws_stride, mi[MI_SLOT_C]); // :1270-1273
            const int sf = mi[MI_SLOT_F];
            ciptr di = dof_map + mi[MI_DOF];
            if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            {
               const SV<T> U = ws_load6(ws, ws_stride, sf);
               const T dinv = MH_WS(sf + 6), u = MH_WS(sf + 7);
               const T qdd = dinv * (u - (dot(U.a, a.a) + dot(U.l, a.l))); // :1280-1282
               orow[di[0] * A.v_es] = qdd;
               if (type == JT_REVOLUTE)
                  a.a.z += qdd;
               else
                  a.l.z += qdd;
            }
            else if (type == JT_PLANAR || type == JT_SPHERICAL)
            { // qdd = D^-1 (u - U^T a')   (:1280-1282)
               const int sl = mi[MI_SLOT_LK];
               const SV<T> U0 = ws_load6(ws, ws_stride, sl), U1 = ws_load6(ws, ws_stride, sl + 6), U2 = ws_load6(ws, ws_stride, sl + 12);
               const S3<T> Di{MH_WS(sl + 18), MH_WS(sl + 19), MH_WS(sl + 20), MH_WS(sl + 21), MH_WS(sl + 22), MH_WS(sl + 23)};
               const V3<T> r{MH_WS(sl + 24) - (dot(U0.a, a.a) + dot(U0.l, a.l)), MH_WS(sl + 25) - (dot(U1.a, a.a) + dot(U1.l, a.l)),
                             MH_WS(sl + 26) - (dot(U2.a, a.a) + dot(U2.l, a.l))};
               const V3<T> qdd = mul(Di, r);
               orow[di[0] * A.v_es] = qdd.x, orow[di[1] * A.v_es] = qdd.y, orow[di[2] * A.v_es] = qdd.z;
               a = a + from_comp3(type, qdd);
            }
            else if (type == JT_SIXDOF)
            {
               const SV<T> x = ws_load6(ws, ws_stride, sf);
               const SV<T> qdd = x - a;
               orow[di[0] * A.v_es] = qdd.a.x, orow[di[1] * A.v_es] = qdd.a.y, orow[di[2] * A.v_es] = qdd.a.z;
               orow[di[3] * A.v_es] = qdd.l.x, orow[di[4] * A.v_es] = qdd.l.y, orow[di[5] * A.v_es] = qdd.l.z;
               a = x;
            }
            if (flags & MF_STORE_VA)
               ws_store6(ws, ws_stride, mi[MI_SLOT_VA], a);
            a_prev = a;
         };
         switch (type_rt)
         {
            case JT_REVOLUTE: body(std::integral_constant<int, JT_REVOLUTE>{}); break;
            case JT_PRISMATIC: body(std::integral_constant<int, JT_PRISMATIC>{}); break;
            case JT_SIXDOF: body(std::integral_constant<int, JT_SIXDOF>{}); break;
            case JT_PLANAR: body(std::integral_constant<int, JT_PLANAR>{}); break;
            case JT_SPHERICAL: body(std::integral_constant<int, JT_SPHERICAL>{}); break;
            default: body(std::integral_constant<int, JT_FIXED>{}); break;
         }
      }
   }
}

#undef MH_WS
} // namespace mh
