// mh_kinematics_vjp_kernels.h -- reverse mode of the kinematics: the gradient of a loss on body poses with respect to q, and J^T w of up to
// sixteen chains without forming J (run-time topology, one lane per configuration, gfx950).
//
// The cotangent of a pose is a wrench on its body; wrenches add up towards the root; each joint reads its share as S_j^T f.  J^T w is
// the map of GeometricJacobianCalculator.getJointTorques (algorithms/GeometricJacobianCalculator.java:477-484), which the reference takes
// through the matrix.
//   sweep  : kin_sweep of mh_kinematics_kernels.h without velocities stores the pose X_j of every canonical after-joint frame in the root
//            body frame (slots 0-11 of the body's KIN_SLOTS).  The six twist slots are free in this call: they hold the wrench that acts on
//            the body and on everything below it, and are zeroed for every configuration (the workspace belongs to the wave).
//   seed   : the cotangent (G_R, g_p) of a pose (R, p) is the wrench (n; f) in the target frame with M = R^T G_R,
//            n = (M32 - M23, M13 - M31, M21 - M12), f = R^T g_p; mh_jacobian_transpose_* reads (n; f) itself.  It is carried into the root
//            body frame through the target's pose and added to the target body's accumulator; with a base that is not the root body the
//            same wrench is taken from the base body's accumulator, so that what both send above their common ancestor cancels.
//   inward : j = n - 1 ... 0.  The accumulated wrench, brought into frame j through the stored pose, gives the joint's entries as its
//            components along the unit twists of the joint kind (dof_comp); then it is added to the parent's accumulator -- plain sums,
//            since all accumulators are in the root body frame.  A child that directly follows its parent hands its wrench over in
//            registers.  A joint on no chain (Euler tour of the tree, as in geometric_jacobian_kernel) gets exact zeros: above a common
//            ancestor the two seeds cancel only to rounding.
// Every entry of the output is written once: the entries of joints on chains, zeros for the others and for the DoF indices no joint owns.
#pragma once
#include "mh_kinematics_kernels.h"

namespace mh
{
template <typename T>
struct KinVjpArgs
{
   Args<T> a;   // m, B, q and its strides, ws
   const T *g;  // pose cotangents [12 K] (K = n_joints with all_bodies) or wrenches [6 K] per configuration with (g_bs, g_es)
   T *out;      // [nv] per configuration with (o_bs, o_es)
   long g_bs, g_es, o_bs, o_es;
   const int *info;                 // [n][RI_STRIDE]: Euler tour of the tree (mh_response_kernels.h)
   const int *zero_ofs, *zero_cols; // the DoF indices no joint owns (mh_gravity_kernels.h)
   int n_targets, all_bodies;
   int tgt[KIN_MAX_TARGETS], base[KIN_MAX_TARGETS]; // engine index of the target's / base's body, -1 = the root body
   T pose[KIN_MAX_TARGETS][12];                     // the target frame in its body's canonical after-joint frame
};

// force vector parent -> child through X (child -> parent pose): f' = R^T f ; n' = R^T (n - p x f)
template <typename T>
MH_DEV SV<T> force_to_child(const XF<T> &X, SV<T> w)
{
   const V3<T> &p = X.p;
   const T tx = w.l.y * p.z - w.l.z * p.y + w.a.x, ty = w.l.z * p.x - w.l.x * p.z + w.a.y, tz = w.l.x * p.y - w.l.y * p.x + w.a.z;
   return SV<T>{tmul(X.R, V3<T>{tx, ty, tz}), tmul(X.R, w.l)};
}
// the wrench (n; f) in the frame at pose X that the cotangent of X's twelve numbers (entry k of the row) stands for
template <typename T>
MH_DEV SV<T> pose_cotangent(const T *row, long es, long k, const XF<T> &X)
{
   const T *g = row + 12 * k * es;
   const M3<T> &R = X.R;
   const V3<T> r1{R.xx, R.yx, R.zx}, r2{R.xy, R.yy, R.zy}, r3{R.xz, R.yz, R.zz};
   const V3<T> g1{g[0], g[3 * es], g[6 * es]}, g2{g[1 * es], g[4 * es], g[7 * es]}, g3{g[2 * es], g[5 * es], g[8 * es]};
   const V3<T> gp{g[9 * es], g[10 * es], g[11 * es]};
   return SV<T>{V3<T>{dot(r3, g2) - dot(r2, g3), dot(r1, g3) - dot(r3, g1), dot(r2, g1) - dot(r1, g2)}, tmul(R, gp)};
}

// WRENCH: G.g holds wrenches in the target frames (mh_jacobian_transpose_*), bases count; otherwise cotangents of poses, every base is the
// root body and G.all_bodies takes the body-fixed frame of every body.
template <typename T, bool WRENCH>
__global__ void __launch_bounds__(256) kinematics_vjp_kernel(KinVjpArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map), dof_map = as_const(m.dof_map), info = as_const(G.info);
   const ciptr zero_ofs = as_const(G.zero_ofs), zero_cols = as_const(G.zero_cols);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64;
   T *ws = A.ws + (lane >> 6) * ((long)m.n * KIN_SLOTS * 64) + (lane & 63);
   const long g_es = G.g_es, o_es = G.o_es;
   const V3<T> Z{T(0), T(0), T(0)};
   const bool all_bodies = !WRENCH && G.all_bodies;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      const T *grow = G.g + cfg * G.g_bs;
      T *orow = G.out + cfg * G.o_bs;
      kin_sweep<T, true>(A, CB, meta, cfg_map, dof_map, qrow, (const T *)nullptr, ws, [&](int j, ciptr mi, const CRef<T> &c, const XF<T> &X) {
         SV<T> W{Z, Z};
         if (all_bodies)
         {
            const XF<T> Xf{M3<T>{c[MC_RF + 0], c[MC_RF + 1], c[MC_RF + 2], c[MC_RF + 3], c[MC_RF + 4], c[MC_RF + 5], c[MC_RF + 6], c[MC_RF + 7], c[MC_RF + 8]},
                           V3<T>{c[MC_PF + 0], c[MC_PF + 1], c[MC_PF + 2]}};
            const XF<T> XT = compose(X, Xf);
            W = force_to_parent(XT, pose_cotangent(grow, g_es, (long)mi[MI_EXT], XT));
         }
         ws_store6(ws, ws_stride, j * KIN_SLOTS + 12, W);
      });
      for (int k = 0; k < (all_bodies ? 0 : G.n_targets); k++)
      {
         const int t = G.tgt[k], b = WRENCH ? G.base[k] : -1;
         if (t == b)
            continue; // the chain is empty (the root body as a target of a pose: nothing moves it)
         XF<T> XT = kin_arg_pose(G.pose[k]);
         if (t >= 0)
            XT = compose(kin_load_pose(ws, ws_stride, t * KIN_SLOTS), XT);
         SV<T> w;
         if (WRENCH)
         {
            const T *g = grow + 6L * k * g_es;
            w = SV<T>{V3<T>{g[0], g[g_es], g[2 * g_es]}, V3<T>{g[3 * g_es], g[4 * g_es], g[5 * g_es]}};
         }
         else
            w = pose_cotangent(grow, g_es, (long)k, XT);
         const SV<T> W = force_to_parent(XT, w);
         if (t >= 0)
            ws_add6(ws, ws_stride, t * KIN_SLOTS + 12, W);
         if (b >= 0)
            ws_add6(ws, ws_stride, b * KIN_SLOTS + 12, T(-1) * W);
      }
      SV<T> carry{Z, Z};
      for (int j = m.n - 1; j >= 0; j--)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS], nd = dof_count(type);
         const SV<T> F = ws_load6(ws, ws_stride, j * KIN_SLOTS + 12) + carry;
         carry = SV<T>{Z, Z};
         if (nd > 0)
         {
            bool on_chain = all_bodies;
            if (!all_bodies)
            {
               const int tin = info[j * RI_STRIDE + RI_TIN], tout = info[j * RI_STRIDE + RI_TOUT];
               for (int k = 0; k < G.n_targets; k++)
               {
                  const int t = G.tgt[k], b = WRENCH ? G.base[k] : -1;
                  const bool above_t = t >= 0 && tin <= info[t * RI_STRIDE + RI_TIN] && info[t * RI_STRIDE + RI_TOUT] <= tout;
                  const bool above_b = b >= 0 && tin <= info[b * RI_STRIDE + RI_TIN] && info[b * RI_STRIDE + RI_TOUT] <= tout;
                  on_chain = on_chain || above_t != above_b;
               }
            }
            ciptr dj = dof_map + mi[MI_DOF];
            if (on_chain)
            {
               const SV<T> fj = force_to_child(kin_load_pose(ws, ws_stride, j * KIN_SLOTS), F);
               for (int d = 0; d < nd; d++)
                  orow[dj[d] * o_es] = comp(fj, dof_comp(type, d));
            }
            else
               for (int d = 0; d < nd; d++)
                  orow[dj[d] * o_es] = T(0);
         }
         if (parent >= 0)
         {
            if (flags & MF_PARENT_ADJ)
               carry = F;
            else
               ws_add6(ws, ws_stride, parent * KIN_SLOTS + 12, F);
         }
      }
      for (int z = zero_ofs[m.n]; z < zero_ofs[m.n + 1]; z++)
         orow[zero_cols[z] * o_es] = T(0); // entries no joint owns
   }
}
} // namespace mh
