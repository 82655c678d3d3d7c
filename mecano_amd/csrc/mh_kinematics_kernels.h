// mh_kinematics_kernels.h -- where the bodies are and how they move with the joints: poses of frames fixed in bodies, geometric Jacobians
// between two bodies and their convective terms (run-time topology, one lane per configuration, gfx950).
//
// Replaces, per configuration, the frame tree's getTransformToDesiredFrame(root body frame) and
// algorithms/GeometricJacobianCalculator.java:148-158 (setKinematicChain), :249-279 (updateJacobianMatrix) and :316-377
// (updateJacobianRateMatrix, computeJacobianRateMatrixBlock) in the engine's canonical joint frames.
//   sweep  : one outward pass composes the pose X_j of every canonical after-joint frame in the root body frame and, when velocities are
//            given, the twist v_j of the body relative to the root body, expressed in frame j.  Both go to the per-wave workspace
//            ([slot][64 lanes], KIN_SLOTS per body).
//   poses  : the pose of a target frame is X_t o (target frame in the canonical frame of its body); the root body's is the frame itself.
//   columns: joint j lies on the chain from the base b to the target t iff exactly one of the two is in its subtree (Euler tour of the
//            tree, a constant of the model).  With t below it the column of DoF k is its unit twist brought from frame j into the target
//            frame through the two stored poses; with b below it the same negated (:268-271: the chain passes the joint from successor to
//            predecessor).  Every other joint gets zeros, so every entry of the block is written exactly once.
//   term   : the reference sums  Jdot_i qd_i  with  Jdot_i = J_i x (twist of the end effector relative to what follows joint i on the chain,
//            :362-377).  With t_i = J_i qd_i that is  sum_i t_i x (v_T - v_i)  for both directions, v_i the stored twist of joint i's
//            successor body and v_T the target's, all in the target frame: behind the common ancestor the difference holds t_i itself,
//            which the cross product with t_i removes.
// Targets are independent after the sweep: gridDim.y waves may share a group of 64 configurations, each redoing the sweep and taking
// every gridDim.y-th target.  The kernels write with (batch stride, entry stride): the host hands them SoA strides always -- into the
// caller's matrix, or into scratch of the context that a transposition brings to AoS rows.
#pragma once
#include "mh_response_kernels.h"

namespace mh
{
#define MH_WS(slot) ws[(long)(slot)*ws_stride]

constexpr int KIN_MAX_TARGETS = 16; // MH_MAX_KINEMATIC_TARGETS
constexpr int KIN_SLOTS = 18;       // per body: pose (R row-major 9, p 3), twist 6

template <typename T>
struct KinArgs
{
   Args<T> a;              // m, B, q, qd (or NULL) and their strides, ws
   T *pose_out;            // [12 K] per configuration with (p_bs, p_es); K = n_joints with all_bodies
   T *J;                   // [6 K][nv] with (j_bs, j_es)
   T *conv;                // [6 K] with (c_bs, c_es), or NULL
   long p_bs, p_es, j_bs, j_es, c_bs, c_es;
   const int *info;        // [n][RI_STRIDE]: Euler tour of the tree (mh_response_kernels.h)
   const int *zero_ofs, *zero_cols; // zero_cols[zero_ofs[n] .. zero_ofs[n + 1]): the DoF indices no joint owns (mh_gravity_kernels.h)
   int n_targets, all_bodies;
   int tgt[KIN_MAX_TARGETS], base[KIN_MAX_TARGETS]; // engine index of the target's / base's body, -1 = the root body
   T pose[KIN_MAX_TARGETS][12]; // the target frame in its body's canonical after-joint frame (root body: in the root body frame)
};

template <typename T>
MH_DEV XF<T> kin_load_pose(const T *ws, long ws_stride, int s)
{
   return XF<T>{M3<T>{MH_WS(s + 0), MH_WS(s + 1), MH_WS(s + 2), MH_WS(s + 3), MH_WS(s + 4), MH_WS(s + 5), MH_WS(s + 6), MH_WS(s + 7), MH_WS(s + 8)},
                V3<T>{MH_WS(s + 9), MH_WS(s + 10), MH_WS(s + 11)}};
}
template <typename T>
MH_DEV void kin_store_pose(T *ws, long ws_stride, int s, const XF<T> &X)
{
   MH_WS(s + 0) = X.R.xx, MH_WS(s + 1) = X.R.xy, MH_WS(s + 2) = X.R.xz, MH_WS(s + 3) = X.R.yx, MH_WS(s + 4) = X.R.yy, MH_WS(s + 5) = X.R.yz;
   MH_WS(s + 6) = X.R.zx, MH_WS(s + 7) = X.R.zy, MH_WS(s + 8) = X.R.zz, MH_WS(s + 9) = X.p.x, MH_WS(s + 10) = X.p.y, MH_WS(s + 11) = X.p.z;
}
template <typename T>
MH_DEV XF<T> kin_arg_pose(const T *ps)
{
   return XF<T>{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
}
template <typename T>
MH_DEV void kin_write_pose(T *row, long es, long k, const XF<T> &X)
{
   T *o = row + 12 * k * es;
   o[0 * es] = X.R.xx, o[1 * es] = X.R.xy, o[2 * es] = X.R.xz, o[3 * es] = X.R.yx, o[4 * es] = X.R.yy, o[5 * es] = X.R.yz;
   o[6 * es] = X.R.zx, o[7 * es] = X.R.zy, o[8 * es] = X.R.zz, o[9 * es] = X.p.x, o[10 * es] = X.p.y, o[11 * es] = X.p.z;
}
// pose of frame j in frame T from their poses in a common frame: x_T = R_T^T (R_j x_j + p_j - p_T)
template <typename T>
MH_DEV XF<T> kin_relative(const XF<T> &XT, const XF<T> &Xj)
{
   const M3<T> &A = XT.R, &B = Xj.R;
   XF<T> o;
   o.R = M3<T>{A.xx * B.xx + A.yx * B.yx + A.zx * B.zx, A.xx * B.xy + A.yx * B.yy + A.zx * B.zy, A.xx * B.xz + A.yx * B.yz + A.zx * B.zz,
               A.xy * B.xx + A.yy * B.yx + A.zy * B.zx, A.xy * B.xy + A.yy * B.yy + A.zy * B.zy, A.xy * B.xz + A.yy * B.yz + A.zy * B.zz,
               A.xz * B.xx + A.yz * B.yx + A.zz * B.zx, A.xz * B.xy + A.yz * B.yy + A.zz * B.zy, A.xz * B.xz + A.yz * B.yz + A.zz * B.zz};
   o.p = tmul(A, Xj.p - XT.p);
   return o;
}

// The outward sweep: X_j = X_parent o X_before o X_joint(q) and v_j = (v_parent in frame j) + S_j qd_j.  STORE_ALL: every body's pose (and
// twist) goes to its slots; otherwise only those a child that does not directly follow its parent reads back.  `visit(j, mi, X)` sees
// every body once, in engine order.
template <typename T, bool STORE_ALL, class VISIT>
MH_DEV void kin_sweep(const Args<T> &A, const T *CB, ciptr meta, ciptr cfg_map, ciptr dof_map, const T *qrow, const T *qdrow, T *ws, VISIT visit)
{
   constexpr long ws_stride = 64;
   const DevModel &m = A.m;
   const V3<T> Z{T(0), T(0), T(0)};
   XF<T> X_prev{M3<T>{T(1), T(0), T(0), T(0), T(1), T(0), T(0), T(0), T(1)}, Z};
   SV<T> v_prev{Z, Z};
   for (int j = 0; j < m.n; j++)
   {
      ciptr mi = meta + j * MI_STRIDE;
      const int parent = mi[MI_PARENT], type = mi[MI_TYPE], flags = mi[MI_FLAGS];
      const CRef<T> c{CB + j * MC_STRIDE};
      const JX<T> jx = joint_from_q<T>(type, cfg_map, mi[MI_CFG], qrow, A.q_es, (T *)nullptr, 0, 0, false);
      XF<T> Xp{M3<T>{T(1), T(0), T(0), T(0), T(1), T(0), T(0), T(0), T(1)}, Z};
      SV<T> vp{Z, Z};
      if (parent >= 0)
      {
         if (flags & MF_PARENT_ADJ)
            Xp = X_prev, vp = v_prev;
         else
         {
            Xp = kin_load_pose(ws, ws_stride, parent * KIN_SLOTS);
            if (qdrow)
               vp = ws_load6(ws, ws_stride, parent * KIN_SLOTS + 12);
         }
      }
      const XF<T> Xb = load_xb<T>(c);
      XF<T> XJ;
      if (general_x(type))
         XJ = jx.X;
      else
      {
         XJ.R = M3<T>{jx.c, -jx.s, T(0), jx.s, jx.c, T(0), T(0), T(0), T(1)};
         XJ.p = V3<T>{T(0), T(0), jx.d};
      }
      const XF<T> X = compose(Xp, compose(Xb, XJ));
      SV<T> v{Z, Z};
      if (qdrow)
         v = motion_down(type, jx, Xb, vp) + joint_vec<T>(type, dof_map, mi[MI_DOF], qdrow, A.v_es, true);
      if (STORE_ALL || (flags & MF_STORE_VA))
      {
         kin_store_pose(ws, ws_stride, j * KIN_SLOTS, X);
         if (qdrow)
            ws_store6(ws, ws_stride, j * KIN_SLOTS + 12, v);
      }
      visit(j, mi, c, X);
      X_prev = X, v_prev = v;
   }
}

// Poses only.  all_bodies: the body-fixed frame of every body, written from the sweep into the row of its joint in the caller's order.
// Otherwise the listed target frames, from the stored poses.
template <typename T>
__global__ void __launch_bounds__(256) body_poses_kernel(KinArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map), dof_map = as_const(m.dof_map);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64;
   T *ws = A.ws + (lane >> 6) * ((long)m.n * KIN_SLOTS * 64) + (lane & 63);
   const long p_es = G.p_es;
   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      T *prow = G.pose_out + cfg * G.p_bs;
      if (G.all_bodies)
      {
         kin_sweep<T, false>(A, CB, meta, cfg_map, dof_map, qrow, (const T *)nullptr, ws, [&](int, ciptr mi, const CRef<T> &c, const XF<T> &X) {
            const XF<T> Xf{M3<T>{c[MC_RF + 0], c[MC_RF + 1], c[MC_RF + 2], c[MC_RF + 3], c[MC_RF + 4], c[MC_RF + 5], c[MC_RF + 6], c[MC_RF + 7], c[MC_RF + 8]},
                           V3<T>{c[MC_PF + 0], c[MC_PF + 1], c[MC_PF + 2]}};
            kin_write_pose(prow, p_es, (long)mi[MI_EXT], compose(X, Xf));
         });
         continue;
      }
      kin_sweep<T, true>(A, CB, meta, cfg_map, dof_map, qrow, (const T *)nullptr, ws, [](int, ciptr, const CRef<T> &, const XF<T> &) {});
      for (int k = 0; k < G.n_targets; k++)
      {
         const int t = G.tgt[k];
         XF<T> XT = kin_arg_pose(G.pose[k]);
         if (t >= 0)
            XT = compose(kin_load_pose(ws, ws_stride, t * KIN_SLOTS), XT);
         kin_write_pose(prow, p_es, (long)k, XT);
      }
   }
}

// Jacobians of the target frames relative to their bases, and their convective terms when G.conv is given (A.qd is then not NULL).
template <typename T>
__global__ void __launch_bounds__(256) geometric_jacobian_kernel(KinArgs<T> G)
{
   const Args<T> &A = G.a;
   const DevModel &m = A.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map), dof_map = as_const(m.dof_map), info = as_const(G.info);
   const ciptr zero_ofs = as_const(G.zero_ofs), zero_cols = as_const(G.zero_cols);
   const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const long nlanes = (long)gridDim.x * blockDim.x;
   constexpr long ws_stride = 64;
   const int part = blockIdx.y, parts = gridDim.y;
   T *ws = A.ws + ((long)part * gridDim.x * (blockDim.x >> 6) + (lane >> 6)) * ((long)m.n * KIN_SLOTS * 64) + (lane & 63);
   const int nv = m.nv;
   const long j_es = G.j_es;
   const V3<T> Z{T(0), T(0), T(0)};
   const bool with_conv = G.conv != nullptr;

   for (long cfg = lane; cfg < A.B; cfg += nlanes)
   {
      const T *qrow = A.q + cfg * A.q_bs;
      const T *qdrow = with_conv ? A.qd + cfg * A.v_bs : nullptr;
      T *Jrow = G.J + cfg * G.j_bs;
      kin_sweep<T, true>(A, CB, meta, cfg_map, dof_map, qrow, qdrow, ws, [](int, ciptr, const CRef<T> &, const XF<T> &) {});
      for (int k = part; k < G.n_targets; k += parts)
      {
         const int t = G.tgt[k], b = G.base[k];
         XF<T> XT = kin_arg_pose(G.pose[k]);
         SV<T> vT{Z, Z};
         if (t >= 0)
         {
            if (with_conv)
               vT = motion_to_child(XT, ws_load6(ws, ws_stride, t * KIN_SLOTS + 12));
            XT = compose(kin_load_pose(ws, ws_stride, t * KIN_SLOTS), XT);
         }
         const int tin_t = t >= 0 ? info[t * RI_STRIDE + RI_TIN] : -1, tout_t = t >= 0 ? info[t * RI_STRIDE + RI_TOUT] : -1;
         const int tin_b = b >= 0 ? info[b * RI_STRIDE + RI_TIN] : -1, tout_b = b >= 0 ? info[b * RI_STRIDE + RI_TOUT] : -1;
         T *Jk = Jrow + 6L * k * nv * j_es; // block k: rows 6 k .. 6 k + 5
         const long rs = (long)nv * j_es;  // from one row of the block to the next
         SV<T> cv{Z, Z};
         for (int j = 0; j < m.n; j++)
         {
            ciptr mi = meta + j * MI_STRIDE;
            const int type = mi[MI_TYPE], nd = dof_count(type);
            if (nd == 0)
               continue;
            ciptr dj = dof_map + mi[MI_DOF];
            const int tin = info[j * RI_STRIDE + RI_TIN], tout = info[j * RI_STRIDE + RI_TOUT];
            const bool above_t = t >= 0 && tin <= tin_t && tout_t <= tout, above_b = b >= 0 && tin <= tin_b && tout_b <= tout;
            if (above_t == above_b)
            { // off the chain: on neither side of the common ancestor, or above it
               for (int d = 0; d < nd; d++)
               {
                  T *o = Jk + dj[d] * j_es;
                  o[0] = T(0), o[rs] = T(0), o[2 * rs] = T(0), o[3 * rs] = T(0), o[4 * rs] = T(0), o[5 * rs] = T(0);
               }
               continue;
            }
            const T sign = above_t ? T(1) : T(-1);
            const XF<T> Xr = kin_relative(XT, kin_load_pose(ws, ws_stride, j * KIN_SLOTS));
            SV<T> tj{Z, Z};
            for (int d = 0; d < nd; d++)
            {
               const SV<T> col = sign * motion_to_parent(Xr, unit_twist<T>(type, d));
               T *o = Jk + dj[d] * j_es;
               o[0] = col.a.x, o[rs] = col.a.y, o[2 * rs] = col.a.z, o[3 * rs] = col.l.x, o[4 * rs] = col.l.y, o[5 * rs] = col.l.z;
               if (with_conv)
                  tj = tj + qdrow[dj[d] * A.v_es] * col;
            }
            if (with_conv)
               cv = cv + crm(tj, vT - motion_to_parent(Xr, ws_load6(ws, ws_stride, j * KIN_SLOTS + 12)));
         }
         for (int z = zero_ofs[m.n]; z < zero_ofs[m.n + 1]; z++)
         { // columns no joint owns
            T *o = Jk + zero_cols[z] * j_es;
            o[0] = T(0), o[rs] = T(0), o[2 * rs] = T(0), o[3 * rs] = T(0), o[4 * rs] = T(0), o[5 * rs] = T(0);
         }
         if (with_conv)
         {
            T *o = G.conv + cfg * G.c_bs + 6L * k * G.c_es;
            const long es = G.c_es;
            o[0] = cv.a.x, o[es] = cv.a.y, o[2 * es] = cv.a.z, o[3 * es] = cv.l.x, o[4 * es] = cv.l.y, o[5 * es] = cv.l.z;
         }
      }
   }
}

#undef MH_WS
} // namespace mh
