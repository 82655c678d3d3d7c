// mh_rnea_deriv_kernels.h -- first-order derivatives of the inverse dynamics with respect to the configuration and the velocities at a
// moving state (run-time topology, one lane per configuration, gfx950), and the product kernel that turns them into the derivatives of
// the forward dynamics.
//
// The reference has no calculator for this; MultiBodyGravityGradientCalculator is the qd = 0, qdd = 0 special case (mh_gravity_kernels.h).
// A step dq of DoF p of joint j is a velocity-space step: the subtree of j moves rigidly by the unit twist s = S_jp while the components
// of qd and qdd stay what they were and the external wrenches stay where they are in the world.  Differentiating the Newton-Euler sweep
// under that motion gives for every body k of the subtree (tests/dynamics_derivatives_check.py states the sums as they stand)
//     dv_k = s x v_k + psid,                  psid  = v_parent(j) x s        (the parent's velocity seen from j: v_j - vJ_j)
//     da_k = s x a_k + psidd + psid x v_k,    psidd = a_parent(j) x s + v_parent(j) x psid
//     df_k = s x* (f_k + fext_k) + I_k psidd + BS_k psid,   BS_k = v x* I - I v x + (I v) xbar*  = B_k + B_k^T + (I_k v_k) xbar*
// with B = v x* I the factorised inertia of the Coriolis kernel and (f xbar*) m := m x* f.  The terms s x (.) are the rigid motion of what
// the body carries; they cancel against the motion of S_i in every effort of the subtree, and what is left sums over subtrees into
// composites: Ic (inertia), Bc (factorised inertia), hc = sum I v (momentum), Fc (force), Wc (external force).  A velocity step gives
//     df_k = BS_k s + I_k (psid + sd),        sd = v_j x s.
// Per DoF (j, p), in frame j:
//     P  = Ic psidd + BSc psid + s x* Wc      own block      d tau_jr / d q_jp  = S_r . P
//     P' = P + s x* Fc                        ancestors a    d tau_ar / d q_jp  = S_r . P'          (P' climbs as a force)
//     Q  = BSc s + Ic (psid + sd)             own + ancestors d tau / d qd_jp   = S_r . Q
//     T1 = Ic s, T4 = BSc^T s, T5 = -s x* Wc  rows of (j, p) at an ancestor a, climbed as forces, with (v x m) . f = -m . (v x* f):
//           d tau_jp / d q_ar  = S_r . (T5 - vl_a x* (T4 - vl_a x* T1) - al_a x* T1)      vl_a, al_a: parent's velocity / acceleration
//           d tau_jp / d qd_ar = S_r . (T4 - (vl_a + v_a) x* T1)                           seen from frame a
// so every entry is a component pick in the canonical joint frames.  Three sweeps: outward (v, a, body force, momentum), inward
// (composites), per DoF the joint's own block and a climb over the ancestors, as gravity_gradient_kernel and crba_kernel walk.
// At qd = 0 every velocity term vanishes and d tau / d qd comes out as exact zeros: consider_coriolis = 0 needs no path of its own.
#pragma once
#include "mh_kernels.h"

namespace mh
{
#define MH_WS(slot) ws[(long)(slot)*ws_stride]

// workspace slots of a body, from DerivArgs::slot[j]: the kernel keeps more per body than the model's common plan has room for
enum : int
{
   DS_JP = 0,  // 2: (cos, sin) of a revolute joint
   DS_F = 2,   // 6: body force, then the subtree's (children add theirs)
   DS_VL = 8,  // 6: the parent's velocity in this frame (v - vJ)
   DS_AL = 14, // 6: the parent's acceleration in this frame
   DS_V = 20,  // 6: velocity
   DS_W = 26,  // 6: external force, then the subtree's
   DS_H = 32,  // 6: momentum I v, then the subtree's
   DS_BC = 38, // 30: composite factorised inertia of the children.  Every body has it: the child that directly follows hands its Bc
               //     through these slots too, not in registers -- 30 numbers less alive during the climbs (with them the fp64 kernel spilled)
   DS_BODY = 68,
   // bodies with a child that does not directly follow them (MF_STORE_VA) only:
   DS_A = 68,  // 6: acceleration, for those children
   DS_IC = 74, // 10: composite inertia accumulator
   DS_BRANCH = 84
};

template <typename T>
struct DerivArgs
{
   Args<T> a;        // m, B, q, qd, in3 = qdd (read only with accel), fext (or NULL), out = tau (or NULL), root acceleration, the switches
   T *dq, *dqd;      // [nv][nv] row-major per configuration, either may be NULL
   long g_bs, g_es;  // batch / entry strides of the two matrices
   const int *slot;  // [n] first workspace slot of every body
   int slots;        // workspace slots per lane
   const int *zero_ofs, *zero_cols; // as in GravArgs
};

// BS m and BS^T m of a composite: B m + B^T m +- m x* h
template <typename T>
MH_DEV SV<T> bs_mul(const FB<T> &B, const SV<T> &h, SV<T> m)
{
   return mul(B, m) + tmul(B, m) + crf(m, h);
}
template <typename T>
MH_DEV SV<T> bs_tmul(const FB<T> &B, const SV<T> &h, SV<T> m)
{
   return mul(B, m) + tmul(B, m) - crf(m, h);
}

template <typename T>
__global__ void __launch_bounds__(256) rnea_derivatives_kernel(DerivArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const ciptr zero_ofs = as_const(G.zero_ofs), zero_cols = as_const(G.zero_cols), slot = as_const(G.slot);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   // gridDim.y waves may share a group of 64 configurations (small batches): each runs the sweeps and takes the rows and columns of every
   // gridDim.y-th body
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)G.slots * 64) + (lane & 63);
   const int nv = m.nv;
   const V3<T> Z{T(0), T(0), T(0)};
   const SV<T> Z6{Z, Z};
   const bool with_ext = A.fext != nullptr, with_tau = A.out != nullptr, with_dq = G.dq != nullptr, with_dqd = G.dqd != nullptr;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = A.qd + cfg * A.v_bs;
      const T *qddrow = A.in3 + cfg * A.v_bs;
      const T *frow = with_ext ? A.fext + cfg * A.f_bs : nullptr;
      T *trow = with_tau ? A.out + cfg * A.v_bs : nullptr;
      T *Dq = with_dq ? G.dq + cfg * G.g_bs : nullptr;
      T *Dv = with_dqd ? G.dqd + cfg * G.g_bs : nullptr;
      const long g_es = G.g_es;
      // ---- outward sweep: velocities, accelerations, the Newton-Euler force and the momentum of every body
      SV<T> v_prev = Z6, a_prev = Z6;
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int s = slot[j];
         SV<T> vp, ap;
         if (parent < 0)
            vp = Z6, ap = root_acceleration(A);
         else if (flags & MF_PARENT_ADJ)
            vp = v_prev, ap = a_prev;
         else
         {
            const int sp = slot[parent];
            vp = ws_load6(ws, ws_stride, sp + DS_V);
            ap = ws_load6(ws, ws_stride, sp + DS_A);
         }
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, s + DS_JP, true);
         const SV<T> vJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, A.coriolis != 0);
         const SV<T> aJ = joint_vec<T>(type, dof_map, mi[MI_DOF], qddrow, A.v_es, A.accel != 0);
         const SV<T> vl = motion_down(type, jx, Xb, vp), al = motion_down(type, jx, Xb, ap);
         const SV<T> v = vl + vJ;
         const SV<T> a = al + aJ + crm(v, vJ);
         const RI<T> I = load_inertia<T>(c);
         const SV<T> h = mul(I, v);
         SV<T> f = mul(I, a) + crf(v, h);
         if (with_ext)
         {
            const SV<T> fe = load_fext<T>(c, frow, A.f_es, mi[MI_EXT]);
            f = f - fe;
            ws_store6(ws, ws_stride, s + DS_W, fe);
         }
         ws_store6(ws, ws_stride, s + DS_F, f);
         ws_store6(ws, ws_stride, s + DS_VL, vl);
         ws_store6(ws, ws_stride, s + DS_AL, al);
         ws_store6(ws, ws_stride, s + DS_V, v);
         ws_store6(ws, ws_stride, s + DS_H, h);
         if (flags & MF_STORE_VA)
            ws_store6(ws, ws_stride, s + DS_A, a);
         v_prev = v, a_prev = a;
      }
      // ---- inward sweep: the composites; the rows and columns of the body's DoFs
      RI<T> rcarry;
      SV<T> fcarry = Z6, wcarry = Z6, hcarry = Z6;
      bool have_carry = false;
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int s = slot[j];
         const SV<T> vj = ws_load6(ws, ws_stride, s + DS_V);
         RI<T> Ic = load_inertia<T>(c);
         FB<T> Bc = fb_from_rigid(Ic, vj);
         SV<T> F = ws_load6(ws, ws_stride, s + DS_F), h = ws_load6(ws, ws_stride, s + DS_H), W = Z6;
         if (with_ext)
            W = ws_load6(ws, ws_stride, s + DS_W);
         if (have_carry)
         {
            add(Ic, rcarry);
            F = F + fcarry, h = h + hcarry, W = W + wcarry;
         }
         if (flags & MF_HAS_ACC)
            add(Ic, ws_load_ri(ws, ws_stride, s + DS_IC));
         if (have_carry || (flags & MF_HAS_ACC))
            add(Bc, ws_load_fb(ws, ws_stride, s + DS_BC));
         have_carry = false;
         const int nd = dof_count(type);
         ciptr dj = dof_map + mi[MI_DOF];
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, s + DS_JP);
         // hand the composites to the parent first: what the climbs below keep alive is then the carry alone
         if (parent >= 0)
         {
            RI<T> Iu = Ic;
            FB<T> Bu = Bc;
            rigid_up(type, jx, Xb, Iu);
            fb_up(type, jx, Xb, Bu);
            const SV<T> Fu = force_up(type, jx, Xb, F), hu = force_up(type, jx, Xb, h);
            SV<T> Wu = Z6;
            if (with_ext)
               Wu = force_up(type, jx, Xb, W);
            const int sp = slot[parent];
            // Bc: the first child to arrive stores, the others add -- the child that directly follows its parent arrives last
            if ((flags & MF_ACC_FIRST) || ((flags & MF_PARENT_ADJ) && !(meta[parent * MI_STRIDE + MI_FLAGS] & MF_HAS_ACC)))
               ws_store_fb(ws, ws_stride, sp + DS_BC, Bu);
            else
            {
               FB<T> bacc = ws_load_fb(ws, ws_stride, sp + DS_BC);
               add(bacc, Bu);
               ws_store_fb(ws, ws_stride, sp + DS_BC, bacc);
            }
            if (flags & MF_PARENT_ADJ)
            {
               rcarry = Iu, fcarry = Fu, hcarry = hu, wcarry = Wu, have_carry = true;
            }
            else
            {
               if (flags & MF_ACC_FIRST)
                  ws_store_ri(ws, ws_stride, sp + DS_IC, Iu);
               else
               {
                  RI<T> acc = ws_load_ri(ws, ws_stride, sp + DS_IC);
                  add(acc, Iu);
                  ws_store_ri(ws, ws_stride, sp + DS_IC, acc);
               }
               ws_add6(ws, ws_stride, sp + DS_F, Fu);
               ws_add6(ws, ws_stride, sp + DS_H, hu);
               if (with_ext)
                  ws_add6(ws, ws_stride, sp + DS_W, Wu);
            }
         }
         const bool mine = j % parts == part;
         if (mine && with_tau)
            for (int k = 0; k < nd; k++)
               trow[dj[k] * A.v_es] = comp(F, dof_comp(type, k));
         if (!mine || !(with_dq || with_dqd))
            continue;
         const SV<T> vl = ws_load6(ws, ws_stride, s + DS_VL), al = ws_load6(ws, ws_stride, s + DS_AL);
         for (int k = 0; k < nd; k++)
         {
            const SV<T> S = unit_twist<T>(type, k);
            const long row = (long)dj[k] * nv;
            const int col = dj[k];
            const SV<T> psid = crm(vl, S);
            const SV<T> psidd = crm(al, S) + crm(vl, psid);
            SV<T> P = mul(Ic, psidd) + bs_mul(Bc, h, psid);
            SV<T> Q = bs_mul(Bc, h, S) + mul(Ic, psid + crm(vj, S));
            SV<T> T1 = mul(Ic, S), T4 = bs_tmul(Bc, h, S), T5 = Z6;
            if (with_ext)
            {
               T5 = crf(S, W);
               P = P + T5;
               T5 = Z6 - T5;
            }
            // the joint's own block
            for (int r = 0; r < nd; r++)
            {
               const int e = dof_comp(type, r);
               if (with_dq)
                  Dq[((long)dj[r] * nv + col) * g_es] = comp(P, e);
               if (with_dqd)
                  Dv[((long)dj[r] * nv + col) * g_es] = comp(Q, e);
            }
            // entries of joints that are neither ancestors nor descendants, and of matrix columns no joint owns
            for (int z = zero_ofs[j]; z < zero_ofs[j + 1]; z++)
            {
               if (with_dq)
                  Dq[(row + zero_cols[z]) * g_es] = T(0);
               if (with_dqd)
                  Dv[(row + zero_cols[z]) * g_es] = T(0);
            }
            P = P + crf(S, F);
            // ancestors: the column of (j, k) from P and Q, its row from T1, T4, T5
            int prev = j, anc = parent;
            XF<T> Xp = Xb;
            JX<T> jp = jx;
            int tp = type;
            while (anc >= 0)
            {
               P = force_up(tp, jp, Xp, P);
               Q = force_up(tp, jp, Xp, Q);
               T1 = force_up(tp, jp, Xp, T1);
               T4 = force_up(tp, jp, Xp, T4);
               if (with_ext)
                  T5 = force_up(tp, jp, Xp, T5);
               ciptr ma = meta + anc * MI_STRIDE;
               const int ta = ma[MI_TYPE], sa = slot[anc];
               ciptr da = dof_map + ma[MI_DOF];
               if (dof_count(ta) > 0)
               {
                  const SV<T> vla = ws_load6(ws, ws_stride, sa + DS_VL), ala = ws_load6(ws, ws_stride, sa + DS_AL);
                  const SV<T> va = ws_load6(ws, ws_stride, sa + DS_V);
                  const SV<T> Gq = T5 - crf(vla, T4 - crf(vla, T1)) - crf(ala, T1);
                  const SV<T> Gv = T4 - crf(vla + va, T1);
                  for (int r = 0; r < dof_count(ta); r++)
                  {
                     const int e = dof_comp(ta, r);
                     if (with_dq)
                     {
                        Dq[((long)da[r] * nv + col) * g_es] = comp(P, e);
                        Dq[(row + da[r]) * g_es] = comp(Gq, e);
                     }
                     if (with_dqd)
                     {
                        Dv[((long)da[r] * nv + col) * g_es] = comp(Q, e);
                        Dv[(row + da[r]) * g_es] = comp(Gv, e);
                     }
                  }
               }
               prev = anc;
               anc = ma[MI_PARENT];
               if (anc >= 0)
               {
                  Xp = load_xb<T>(CRef<T>{CB + prev * MC_STRIDE});
                  jp = joint_again<T>(ta, cfg_map, ma[MI_CFG], qrow, A.q_es, ws, ws_stride, sa + DS_JP);
                  tp = ta;
               }
            }
         }
      }
      // matrix rows (and effort entries) no joint owns
      if (part == 0)
         for (int z = zero_ofs[m.n]; z < zero_ofs[m.n + 1]; z++)
         {
            const int r = zero_cols[z];
            if (with_tau)
               trow[r * A.v_es] = T(0);
            for (int cidx = 0; cidx < nv; cidx++)
            {
               if (with_dq)
                  Dq[((long)r * nv + cidx) * g_es] = T(0);
               if (with_dqd)
                  Dv[((long)r * nv + cidx) * g_es] = T(0);
            }
         }
   }
}

// D <- -Hinv D for up to two matrices D of every configuration, in place: one workgroup per configuration; a chunk of kc columns of D
// goes to LDS (kc * nv entries, whatever nv is), every thread then forms entries of those columns of the product and writes them back
// over the chunk -- column k of the product depends on column k of D alone.  Hinv is read as its transpose (the matrix is symmetric;
// the device's differs from its transpose by rounding), which makes the reads of neighbouring threads neighbours in the AoS layout.
template <typename T>
struct NegSolveArgs
{
   const T *Hinv;
   T *D0, *D1; // D1 may be NULL
   long B, bs, es;
   int nv, kc;
};
constexpr int NEG_SOLVE_LDS_ENTRIES = 4096;
template <typename T>
__global__ void __launch_bounds__(256) neg_hinv_product_kernel(NegSolveArgs<T> A)
{
   __shared__ T colbuf[NEG_SOLVE_LDS_ENTRIES];
   const int nv = A.nv, kc = A.kc, t = threadIdx.x, nt = blockDim.x;
   for (long cfg = blockIdx.x; cfg < A.B; cfg += gridDim.x)
   {
      const T *H = A.Hinv + cfg * A.bs;
      for (int which = 0; which < 2; which++)
      {
         T *D = which == 0 ? A.D0 : A.D1;
         if (!D)
            continue;
         D += cfg * A.bs;
         for (int k0 = 0; k0 < nv; k0 += kc)
         {
            const int nk = min(kc, nv - k0);
            __syncthreads();
            for (int idx = t; idx < nv * nk; idx += nt)
            {
               const int j = idx / nk, k = idx - j * nk;
               colbuf[k * nv + j] = D[((long)j * nv + k0 + k) * A.es];
            }
            __syncthreads();
            for (int idx = t; idx < nv * nk; idx += nt)
            {
               const int k = idx / nv, i = idx - k * nv;
               const T *cb = colbuf + k * nv;
               T acc = T(0);
               for (int j = 0; j < nv; j++)
                  acc += H[((long)j * nv + i) * A.es] * cb[j];
               D[((long)i * nv + k0 + k) * A.es] = -acc;
            }
         }
      }
   }
}

#undef MH_WS
} // namespace mh
