// mh_gravity_kernels.h -- joint efforts that hold the system against gravity and external wrenches, and their gradient with respect to
// the configuration (run-time topology, one lane per configuration, gfx950).
//
// Replaces, per configuration, algorithms/MultiBodyGravityGradientCalculator.java:397-672 (passOne, passTwo and the element formulas) in
// the engine's canonical joint frames.  The reference evaluates every entry of the gradient from the subtree's gravity force f = -m g at
// its centre of mass c and, for the external part, by a recursion over every wrench of the subtree.  Both collapse (tests/
// gravity_gradient_check.py restates the reference entry by entry; the device is compared against it):
//   gravity   : with h = m c the subtree's first moment and S_o = (w_o, v_o) a unit twist of body j, the entry of the pair (o, ancestor a)
//               is w_a . A_o,  A_o = -(m v_o + w_o x h) x g_j  -- a pure couple, so the climb to the ancestors only rotates it, and
//               prismatic ancestors get zeros.  No division by the subtree mass.
//   external  : the sum over the wrenches of the subtree is  S_a . (-S_o x* W_j),  W_j the subtree's external spatial force in frame j --
//               a spatial force that force_up carries to the ancestors.
// so that  grad[o][a] = S_a . F_o  with  F_o = (A_o, 0) - S_o x* W_j  (d tau_o / d q_a: the wrenches stay fixed in the world) and
// grad[a][o] = w_a . A_o (gravity only), and inside a joint grad[o][r] = S_r . F_o for every pair of its DoFs.
// Three sweeps: gravity handed down as a 3-vector (rotations only); first moment and external force handed up; per DoF the entries of
// the joint's own block and a climb over the ancestors, as crba_kernel walks for H.  Subtree masses are constants of the model.
#pragma once
#include "mh_kernels.h"

namespace mh
{
#define MH_WS(slot) ws[(long)(slot)*ws_stride]

template <typename T>
struct GravArgs
{
   Args<T> a;         // m, B, q, fext (or NULL), out = tau (or NULL), outb = grad (or NULL), the strides of q / tau / fext, (gx, gy, gz) = gravity
   long g_bs, g_es;   // batch / entry strides of grad ([nv][nv] row-major per configuration)
   const T *sub_mass; // [n] mass of the subtree of every body (engine order)
   // entries no pair of related joints owns, so that the kernel writes the whole matrix: for body j the DoF indices zero_cols[zero_ofs[j]
   // .. zero_ofs[j + 1]) of every joint that is neither j, an ancestor nor a descendant of j (and of matrix rows no joint owns);
   // zero_ofs[n] .. zero_ofs[n + 1]: the matrix rows no joint owns
   const int *zero_ofs, *zero_cols;
};

// a free 3-vector from the parent's after-joint frame into this joint's, and back
template <typename T>
MH_DEV V3<T> rotate_down(int type, const JX<T> &jx, const M3<T> &Rb, V3<T> v)
{
   v = tmul(Rb, v);
   if (type == JT_REVOLUTE)
      return rotzT(jx.c, jx.s, v);
   if (general_x(type))
      return tmul(jx.X.R, v);
   return v;
}
template <typename T>
MH_DEV V3<T> rotate_up(int type, const JX<T> &jx, const M3<T> &Rb, V3<T> v)
{
   if (type == JT_REVOLUTE)
      v = rotz(jx.c, jx.s, v);
   else if (general_x(type))
      v = mul(jx.X.R, v);
   return mul(Rb, v);
}
// first moment h = m c of a subtree of mass m, child -> parent: h' = R h + m p through the joint and the constant pose
template <typename T>
MH_DEV V3<T> first_moment_up(int type, const JX<T> &jx, const XF<T> &Xb, V3<T> h, T m)
{
   if (type == JT_REVOLUTE)
      h = rotz(jx.c, jx.s, h);
   else if (type == JT_PRISMATIC)
      h.z += m * jx.d;
   else if (general_x(type))
      h = mul(jx.X.R, h) + m * jx.X.p;
   return mul(Xb.R, h) + m * Xb.p;
}

// per-body workspace: MI_SLOT_F + 0..5 subtree external force (accumulated), MI_SLOT_C + 0..2 gravity in the body's frame,
// MI_SLOT_C + 3..5 subtree first moment (accumulated); (cos, sin) of revolute joints in MI_SLOT_JP as everywhere
template <typename T>
__global__ void __launch_bounds__(256) gravity_gradient_kernel(GravArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map), cfg_map = as_const(m.cfg_map);
   const ciptr zero_ofs = as_const(G.zero_ofs), zero_cols = as_const(G.zero_cols);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64; // [slot][64 lanes] per wave, as in the other sweep kernels
   // gridDim.y waves may share a group of 64 configurations (small batches): each runs the sweeps and takes the rows and columns of every
   // gridDim.y-th body
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)m.n_slots * 64) + (lane & 63);
   const int nv = m.nv;
   const V3<T> Z{T(0), T(0), T(0)};
   const bool with_ext = A.fext != nullptr, with_grad = A.outb != nullptr, with_tau = A.out != nullptr;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      const T *frow = with_ext ? A.fext + cfg * A.f_bs : nullptr;
      T *trow = with_tau ? A.out + cfg * A.v_bs : nullptr;
      T *Gm = with_grad ? A.outb + cfg * G.g_bs : nullptr;
      const long g_es = G.g_es;
      // ---- outward sweep: joint transforms, gravity in every frame; each body's own first moment and external force
      V3<T> g_prev = Z;
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP], true);
         V3<T> gp;
         if (parent < 0)
            gp = V3<T>{A.gx, A.gy, A.gz};
         else if (flags & MF_PARENT_ADJ)
            gp = g_prev;
         else
         {
            const int sp = meta[parent * MI_STRIDE + MI_SLOT_C];
            gp = V3<T>{MH_WS(sp + 0), MH_WS(sp + 1), MH_WS(sp + 2)};
         }
         const XF<T> Xb = load_xb<T>(c);
         const V3<T> g = rotate_down(type, jx, Xb.R, gp);
         const int sc = mi[MI_SLOT_C];
         MH_WS(sc + 0) = g.x, MH_WS(sc + 1) = g.y, MH_WS(sc + 2) = g.z;
         MH_WS(sc + 3) = c[MC_H + 0], MH_WS(sc + 4) = c[MC_H + 1], MH_WS(sc + 5) = c[MC_H + 2];
         if (with_ext)
            ws_store6(ws, ws_stride, mi[MI_SLOT_F], load_fext<T>(c, frow, A.f_es, mi[MI_EXT]));
         g_prev = g;
      }
      // ---- inward sweep: subtree first moment and external force; the rows and columns of the body's DoFs
      V3<T> h_carry = Z;
      SV<T> w_carry{Z, Z};
      bool have_carry = false;
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
         const CRef<T> c{CB + j * MC_STRIDE};
         const int sc = mi[MI_SLOT_C];
         const V3<T> g{MH_WS(sc + 0), MH_WS(sc + 1), MH_WS(sc + 2)};
         V3<T> h{MH_WS(sc + 3), MH_WS(sc + 4), MH_WS(sc + 5)};
         SV<T> W{Z, Z};
         if (with_ext)
            W = ws_load6(ws, ws_stride, mi[MI_SLOT_F]);
         if (have_carry)
         {
            h = h + h_carry;
            W = W + w_carry;
         }
         have_carry = false;
         const T ms = ldc(G.sub_mass + j);
         const int nd = dof_count(type);
         ciptr dj = dof_map + mi[MI_DOF];
         const XF<T> Xb = load_xb<T>(c);
         const JX<T> jx = joint_again<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, ws, ws_stride, mi[MI_SLOT_JP]);
         const bool mine = j % parts == part;
         if (mine && with_tau)
         { // the wrench the joint holds: (-h x g - n_ext, -m g - f_ext)   (computeTauElement, :541-563)
            const SV<T> Wt = SV<T>{cross(g, h), (T(0) - ms) * g} - W;
            for (int k = 0; k < nd; k++)
               trow[dj[k] * A.v_es] = comp(Wt, dof_comp(type, k));
         }
         for (int k = 0; k < ((mine && with_grad) ? nd : 0); k++)
         {
            const SV<T> S = unit_twist<T>(type, k);
            const long row = (long)dj[k] * nv;
            V3<T> Ao = cross(g, ms * S.l + cross(S.a, h)); // -(m v + w x h) x g
            SV<T> F{Ao, Z};
            if (with_ext)
               F = F - crf(S, W);
            // the joint's own block (:491-509): grad[o][r] = S_r . F_o
            for (int r = 0; r < nd; r++)
               Gm[(row + dj[r]) * g_es] = comp(F, dof_comp(type, r));
            // entries of joints that are neither ancestors nor descendants, and of matrix columns no joint owns
            for (int z = zero_ofs[j]; z < zero_ofs[j + 1]; z++)
               Gm[(row + zero_cols[z]) * g_es] = T(0);
            // ancestors (:511-538): grad[o][a] = S_a . F_o, grad[a][o] = w_a . A_o
            int prev = j, anc = parent;
            XF<T> Xp = Xb;
            JX<T> jp = jx;
            int tp = type;
            while (anc >= 0)
            {
               Ao = rotate_up(tp, jp, Xp.R, Ao);
               if (with_ext)
                  F = force_up(tp, jp, Xp, F);
               ciptr ma = meta + anc * MI_STRIDE;
               const int ta = ma[MI_TYPE];
               ciptr da = dof_map + ma[MI_DOF];
               for (int r = 0; r < dof_count(ta); r++)
               {
                  const int e = dof_comp(ta, r);
                  const T sym = e == 0 ? Ao.x : e == 1 ? Ao.y : e == 2 ? Ao.z : T(0);
                  Gm[((long)da[r] * nv + dj[k]) * g_es] = sym;
                  Gm[(row + da[r]) * g_es] = with_ext ? comp(F, e) : sym;
               }
               prev = anc;
               anc = ma[MI_PARENT];
               if (anc >= 0)
               {
                  Xp = load_xb<T>(CRef<T>{CB + prev * MC_STRIDE});
                  jp = joint_again<T>(ta, cfg_map, ma[MI_CFG], qrow, A.q_es, ws, ws_stride, ma[MI_SLOT_JP]);
                  tp = ta;
               }
            }
         }
         if (parent >= 0)
         {
            const V3<T> hp = first_moment_up(type, jx, Xb, h, ms);
            SV<T> Wp{Z, Z};
            if (with_ext)
               Wp = force_up(type, jx, Xb, W);
            if (flags & MF_PARENT_ADJ)
            {
               h_carry = hp, w_carry = Wp, have_carry = true;
            }
            else
            {
               const int sp = meta[parent * MI_STRIDE + MI_SLOT_C];
               MH_WS(sp + 3) += hp.x, MH_WS(sp + 4) += hp.y, MH_WS(sp + 5) += hp.z;
               if (with_ext)
                  ws_add6(ws, ws_stride, meta[parent * MI_STRIDE + MI_SLOT_F], Wp);
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
            for (int cidx = 0; with_grad && cidx < nv; cidx++)
               Gm[((long)r * nv + cidx) * g_es] = T(0);
         }
   }
}

#undef MH_WS
} // namespace mh
