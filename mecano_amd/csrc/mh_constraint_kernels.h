// mh_constraint_kernels.h -- the equality-constrained solve between two forward-dynamics launches (run-time topology, one lane per
// configuration, gfx950): mh_aba_constrained_* and mh_constraint_impulse_*.
//
// K target frames, each with a 6-bit row mask (rows 0-2 angular, 3-5 linear), m selected rows in all.  Per configuration:
//   1. right-hand side  b = des - (motion of the target frame relative to the root body, in the target frame), selected rows only.
//      Acceleration form: the per-body accelerations of the free forward dynamics (relative to the inertial frame, body-fixed frames) minus
//      the root acceleration brought to the body -- RigidBodyAccelerationProvider.getRelativeAcceleration(root, body), which with a base
//      at rest is a plain change of frame (relative_acceleration_kernel, b1 = -1) -- then the constant target pose.  This is J qdd + Jdot qd
//      of mh_geometric_jacobian_* with every base at the root.  Velocity form: the per-body twists, which are relative to the root already.
//   2. A = the selected rows and columns of W + eps I, W = J H^-1 J^T from apparent_inertia_kernel (COUPLED) in SoA scratch.  A row that
//      is inactive in this configuration gets a unit diagonal, zero off-diagonals and a zero right-hand side: m, and with it the control
//      flow, is the same for every lane.
//   3. A = L D L^T in place in the lower triangle of W (row by row; 1 / d on the diagonal), the forward substitution riding along, then the
//      back substitution: lambda.  Nothing of the system lives in registers: an m = 48 system has 1 176 entries.  W is [(6 K)^2][B], so
//      every access is contiguous across lanes, as are those of the right-hand side ([6 K][B] scratch behind W).
//   4. lambda_out (zeros in unselected and inactive rows), and the complete wrench matrix of the second forward-dynamics launch in the
//      call's layout: f_ext (or 0) of every body plus X_k^T lambda_k of the targets on it (force transform of the target pose).
// A pivot that is not positive and finite makes every output of that configuration a quiet NaN: lambda directly, the accelerations
// through a NaN in every wrench of the row.  The test reads the pivot's bits: the translation unit is compiled with -ffinite-math-only.
//
// REL = true: mh_aba_constrained_between_* and mh_constraint_impulse_between_*, where target frame k is held relative to the body of
// base[k] (the root where base[k] < 0, with the arithmetic above).  A second instantiation: the rooted one keeps its code.
//   0. Z_k, the pose of target frame k in the body-fixed frame of its base, from two climbs to the root (body_pose_in_root); parked in
//      scratch ([12 K][B]) for steps 2 and 4.
//   1. acceleration form: the acceleration of the target body relative to the base body with the arithmetic of
//      relative_acceleration_kernel, velocity terms included (per-body twists of the free launch), then the target pose; velocity form:
//      X_k v_t - Z_k v_b.
//   2. W arrives for n_app = K + (non-root bases) frames: the K target frames, then every non-root base's body-fixed frame.  With
//      J_rel,k = J_t - Z_k J_b every block pair k >= l becomes, in place over W[t_k, t_l],
//         W[t_k, t_l] - Z_k W[b_k, t_l] - W[t_k, b_l] Z_l^T + Z_k W[b_k, b_l] Z_l^T
//      (first the columns of [W[t_k, t_l]  W[t_k, b_l]] minus Z_k times those of the base's rows, then the rows of the first minus Z_l times
//      those of the second; W[t_k, b_l] is read by this pair alone, so it is the scratch of the first stage).  The factorisation then
//      runs on the leading blocks with ld = 6 n_app and the same index list.
//   4. the base body receives -Z_k^T lambda_k.
#pragma once
#include "mh_kernels.h"

namespace mh
{
constexpr int CON_MAX_TARGETS = 8; // MH_MAX_CONSTRAINT_TARGETS
constexpr int CON_MAX_ROWS = 6 * CON_MAX_TARGETS;

template <typename T>
struct ConArgs
{
   DevModel m;
   long B;
   const T *q;          // rooted targets: acceleration form only (the root acceleration is brought to the bodies)
   long q_bs, q_es;
   const T *body;       // [B][n_joints][6] with (f_bs, f_es): per-body accelerations (acceleration form) or twists (velocity form)
   const T *fext;       // caller's external wrenches with (f_bs, f_es), or NULL
   T *wrench;           // [B][n_joints][6] with (f_bs, f_es): what the second forward-dynamics launch reads
   long f_bs, f_es;
   T *W;                // [(6 K)^2][B]: W in, its factor out
   T *rhs;              // [m][B]: right-hand side, then lambda (selected rows, packed)
   const int *active;   // [B][K] with (a_bs, a_es), or NULL = every row active
   long a_bs, a_es;
   const T *des;        // [B][K][6] with (d_bs, d_es), or NULL = zeros
   T *lambda;           // same shape and strides, or NULL
   long d_bs, d_es;
   T eps;
   T gx, gy, gz, rax, ray, raz; // root acceleration (root_acceleration()); velocity form: unused
   int K, rows_total, velocity;
   int tgt[CON_MAX_TARGETS];     // engine index of the target's body
   int ext[CON_MAX_TARGETS];     // its joint in the caller's order (rows of body / fext / wrench)
   int rows[CON_MAX_TARGETS];    // 6-bit row mask
   signed char idx[CON_MAX_ROWS]; // row / column of W of selected row a
   T pose[CON_MAX_TARGETS][12];  // the target frame in the body-fixed frame (R row-major, p)
};

// the relative form's additions
template <typename T>
struct ConRelArgs : ConArgs<T>
{
   const T *twist;               // acceleration form: per-body twists of the free launch, laid out as `body` (velocity form: body holds them)
   T *zpose;                     // [12 K][B]: Z_k of the targets with a non-root base
   int n_app;                    // frames of W: K targets, then the non-root bases
   int base[CON_MAX_TARGETS];    // engine index of the base's body, -1 = the root body
   int bext[CON_MAX_TARGETS];    // its joint in the caller's order
   int bslot[CON_MAX_TARGETS];   // its frame in W (>= K), -1 = the root body
};

// pose of frame j in frame t from their poses in a common frame: x_t = R_t^T (R_j x_j + p_j - p_t)
template <typename T>
MH_DEV XF<T> con_relative(const XF<T> &Xt, const XF<T> &Xj)
{
   const M3<T> &A = Xt.R, &B = Xj.R;
   XF<T> o;
   o.R = M3<T>{A.xx * B.xx + A.yx * B.yx + A.zx * B.zx, A.xx * B.xy + A.yx * B.yy + A.zx * B.zy, A.xx * B.xz + A.yx * B.yz + A.zx * B.zz,
               A.xy * B.xx + A.yy * B.yx + A.zy * B.zx, A.xy * B.xy + A.yy * B.yy + A.zy * B.zy, A.xy * B.xz + A.yy * B.yz + A.zy * B.zz,
               A.xz * B.xx + A.yz * B.yx + A.zz * B.zx, A.xz * B.xy + A.yz * B.yy + A.zz * B.zy, A.xz * B.xz + A.yz * B.yz + A.zz * B.zz};
   o.p = tmul(A, Xj.p - Xt.p);
   return o;
}
template <typename T>
MH_DEV XF<T> con_load_pose(const T *z, long B)
{
   return XF<T>{M3<T>{z[0], z[B], z[2 * B], z[3 * B], z[4 * B], z[5 * B], z[6 * B], z[7 * B], z[8 * B]}, V3<T>{z[9 * B], z[10 * B], z[11 * B]}};
}
// x[0 .. 5] (stride s) -= Z (x'[0 .. 5], stride s), both motion vectors
template <typename T>
MH_DEV void con_sub_moved(const XF<T> &Z, T *x, const T *from, long s)
{
   const SV<T> v = motion_to_child(Z, SV<T>{V3<T>{from[0], from[s], from[2 * s]}, V3<T>{from[3 * s], from[4 * s], from[5 * s]}});
   x[0] -= v.a.x, x[s] -= v.a.y, x[2 * s] -= v.a.z, x[3 * s] -= v.l.x, x[4 * s] -= v.l.y, x[5 * s] -= v.l.z;
}

// W = J H^-1 J^T of n_app = ld / 6 frames (the K target frames, then the body-fixed frames of the non-root bases; bslot[k] the frame of
// target k's base, -1 = the root body) becomes that of the relative motions J_rel,k = J_t - Z_k J_b, block pair by block pair with k >= l, in
// place over the targets' blocks (the header's step 2).  W and zpose are the lane's own: entries B apart, Z_k at zpose + 12 k B.  (The
// six-fold loops stay rolled: unrolled, their loads in flight take the constraint kernel from 202 to 256 + 14 registers in fp64, one wave
// per SIMD.)
template <typename T>
MH_DEV void con_reduce_relative(T *W, const T *zpose, long B, long ld, int K, const int *bslot)
{
   const long cs = ld * B; // from one row of W to the next
   for (int k = 0; k < K; k++)
      for (int l = 0; l <= k; l++)
      {
         const int bk = bslot[k], bl = bslot[l];
         T *Wtt = W + (6L * k * ld + 6L * l) * B;
         T *Wtb = bl >= 0 ? W + (6L * k * ld + 6L * bl) * B : nullptr;
         if (bk >= 0)
         {
            const XF<T> Zk = con_load_pose(zpose + 12L * k * B, B);
            const T *Wbt = W + (6L * bk * ld + 6L * l) * B;
#pragma nounroll
            for (int c = 0; c < 6; c++)
               con_sub_moved(Zk, Wtt + c * B, Wbt + c * B, cs);
            if (bl >= 0)
            {
               const T *Wbb = W + (6L * bk * ld + 6L * bl) * B;
#pragma nounroll
               for (int c = 0; c < 6; c++)
                  con_sub_moved(Zk, Wtb + c * B, Wbb + c * B, cs);
            }
         }
         if (bl >= 0)
         {
            const XF<T> Zl = con_load_pose(zpose + 12L * l * B, B);
#pragma nounroll
            for (int r = 0; r < 6; r++)
               con_sub_moved(Zl, Wtt + r * cs, Wtb + r * cs, B);
         }
      }
}

// wrench row of joint `ext` (entries es apart) += X^T lam: lam acts at and in the frame at `ps` (R row-major, p) of that joint's body
template <typename T>
MH_DEV void con_add_wrench(T *wrow, int ext, long es, const T *ps, const SV<T> &lam)
{
   const XF<T> Xt{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
   const SV<T> f = force_to_parent(Xt, lam);
   T *o = wrow + (long)ext * 6 * es; // (two targets on one body: the lane reads back its own store)
   o[0] += f.a.x, o[es] += f.a.y, o[2 * es] += f.a.z, o[3 * es] += f.l.x, o[4 * es] += f.l.y, o[5 * es] += f.l.z;
}

MH_DEV bool pivot_ok(double d)
{
   const long long b = __double_as_longlong(d);
   return b > 0 && b < 0x7ff0000000000000ll;
}
MH_DEV bool pivot_ok(float d)
{
   const int b = __float_as_int(d);
   return b > 0 && b < 0x7f800000;
}
MH_DEV double quiet_nan(double) { return __longlong_as_double(0x7ff8000000000000ll); }
MH_DEV float quiet_nan(float) { return __int_as_float(0x7fc00000); }

template <typename T, bool REL = false>
__global__ void __launch_bounds__(64) constraint_solve_kernel(std::conditional_t<REL, ConRelArgs<T>, ConArgs<T>> G)
{
   const DevModel &m = G.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map);
   const long nlanes = (long)gridDim.x * blockDim.x;
   long ld = 6L * G.K;
   if constexpr (REL)
      ld = 6L * G.n_app;
   const long B = G.B;
   const int K = G.K, M = G.rows_total;

   for (long cfg = (long)blockIdx.x * blockDim.x + threadIdx.x; cfg < B; cfg += nlanes)
   {
      T *W = G.W + cfg, *rhs = G.rhs + cfg;
      const T *brow = G.body + cfg * G.f_bs;
      // ---- 1. right-hand side and the lane's active rows (bit a: selected row a takes part)
      unsigned long long act = 0ull;
      for (int k = 0, a = 0; k < K; k++)
      {
         const int rk = G.rows[k];
         const int ak = G.active ? G.active[cfg * G.a_bs + k * G.a_es] : 0x3f;
         const long e = (long)G.ext[k] * 6;
         SV<T> v{V3<T>{brow[(e + 0) * G.f_es], brow[(e + 1) * G.f_es], brow[(e + 2) * G.f_es]},
                 V3<T>{brow[(e + 3) * G.f_es], brow[(e + 4) * G.f_es], brow[(e + 5) * G.f_es]}};
         bool rooted = true;
         if constexpr (REL)
            if (G.base[k] >= 0)
            { // ---- 0. + 1. against a moving base
               rooted = false;
               const T *ps = G.pose[k];
               const XF<T> Xt{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
               const T *qrow = G.q + cfg * G.q_bs;
               const XF<T> X_b = body_pose_in_root<T>(m, meta, cfg_map, CB, qrow, G.q_es, G.base[k]);
               const XF<T> X12 = con_relative(body_pose_in_root<T>(m, meta, cfg_map, CB, qrow, G.q_es, G.tgt[k]), X_b); // base's frame in the target body's
               const XF<T> Z = con_relative(X12, Xt);
               T *z = G.zpose + 12L * k * B + cfg;
               z[0] = Z.R.xx, z[B] = Z.R.xy, z[2 * B] = Z.R.xz, z[3 * B] = Z.R.yx, z[4 * B] = Z.R.yy, z[5 * B] = Z.R.yz;
               z[6 * B] = Z.R.zx, z[7 * B] = Z.R.zy, z[8 * B] = Z.R.zz, z[9 * B] = Z.p.x, z[10 * B] = Z.p.y, z[11 * B] = Z.p.z;
               const long eb = (long)G.bext[k] * 6;
               auto load6 = [&](const T *row, long at) {
                  return SV<T>{V3<T>{row[(at + 0) * G.f_es], row[(at + 1) * G.f_es], row[(at + 2) * G.f_es]},
                               V3<T>{row[(at + 3) * G.f_es], row[(at + 4) * G.f_es], row[(at + 5) * G.f_es]}};
               };
               if (G.velocity)
                  v = motion_to_child(Xt, v) - motion_to_child(Z, load6(brow, eb));
               else
               { // relative_acceleration_kernel with (b1, b2) = (base, target body)
                  const T *trow = G.twist + cfg * G.f_bs;
                  const SV<T> t1 = load6(trow, eb), t2 = load6(trow, e);
                  SV<T> a1 = load6(brow, eb);
                  const SV<T> d = t1 - motion_to_child(X12, t2);
                  a1.l = a1.l + cross(d.l, t1.a) + cross(d.a, t1.l);
                  a1.a = a1.a + cross(d.a, t1.a);
                  v = motion_to_child(Xt, v - motion_to_parent(X12, a1));
               }
            }
         if (rooted)
         {
            if (!G.velocity)
            {
               const XF<T> Xb = body_pose_in_root<T>(m, meta, cfg_map, CB, G.q + cfg * G.q_bs, G.q_es, G.tgt[k]);
               v = v - motion_to_child(Xb, root_acceleration(G));
            }
            const T *ps = G.pose[k];
            const XF<T> Xt{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
            v = motion_to_child(Xt, v);
         }
         const T free6[6] = {v.a.x, v.a.y, v.a.z, v.l.x, v.l.y, v.l.z};
#pragma unroll
         for (int r = 0; r < 6; r++)
            if ((rk >> r) & 1)
            {
               const T want = G.des ? G.des[cfg * G.d_bs + (6L * k + r) * G.d_es] : T(0);
               const bool on = (ak >> r) & 1;
               rhs[(long)a * B] = on ? want - free6[r] : T(0);
               act |= (unsigned long long)on << a;
               a++;
            }
      }
      if constexpr (REL) // ---- 2. W of the relative motions, in place over the targets' blocks
         con_reduce_relative(W, G.zpose + cfg, B, ld, K, G.bslot);
      // ---- 2. + 3. L D L^T of the masked system, row by row, in place; y = L^-1 b rides along
      bool bad = false;
      for (int i = 0; i < M; i++)
      {
         const long pi = (long)G.idx[i] * ld;
         const bool ai = (act >> i) & 1;
         for (int j = 0; j < i; j++)
         {
            const long pj = (long)G.idx[j] * ld;
            T *wij = W + (pi + G.idx[j]) * B;
            T t = ai && ((act >> j) & 1) ? *wij : T(0);
            for (int k = 0; k < j; k++) // W[i][k] still holds t_ik = l_ik d_k here; W[j][k] holds l_jk
               t -= W[(pi + G.idx[k]) * B] * W[(pj + G.idx[k]) * B];
            *wij = t;
         }
         T *wii = W + (pi + G.idx[i]) * B;
         T d = ai ? *wii + G.eps : T(1);
         T y = rhs[(long)i * B];
         for (int k = 0; k < i; k++)
         {
            T *wik = W + (pi + G.idx[k]) * B;
            const T t = *wik, l = t * W[((long)G.idx[k] * ld + G.idx[k]) * B];
            d -= t * l;
            y -= l * rhs[(long)k * B];
            *wik = l;
         }
         bad = bad || !pivot_ok(d);
         *wii = T(1) / d;
         rhs[(long)i * B] = y;
      }
      for (int i = M - 1; i >= 0; i--)
      {
         T x = rhs[(long)i * B] * W[((long)G.idx[i] * ld + G.idx[i]) * B];
         for (int k = i + 1; k < M; k++)
            x -= W[((long)G.idx[k] * ld + G.idx[i]) * B] * rhs[(long)k * B];
         rhs[(long)i * B] = x;
      }
      // ---- 4. lambda_out and the wrenches of the second launch
      const T nan = quiet_nan(T(0));
      T *wrow = G.wrench + cfg * G.f_bs;
      const T *frow = G.fext ? G.fext + cfg * G.f_bs : nullptr;
      for (long e = 0; e < 6L * m.n; e++)
         wrow[e * G.f_es] = bad ? nan : frow ? frow[e * G.f_es] : T(0);
      for (int k = 0, a = 0; k < K; k++)
      {
         const int rk = G.rows[k];
         T lam[6];
#pragma unroll
         for (int r = 0; r < 6; r++)
         {
            lam[r] = T(0);
            if ((rk >> r) & 1)
            {
               if ((act >> a) & 1)
                  lam[r] = rhs[(long)a * B];
               a++;
            }
            if (bad)
               lam[r] = nan;
            if (G.lambda)
               G.lambda[cfg * G.d_bs + (6L * k + r) * G.d_es] = lam[r];
         }
         const long es = G.f_es;
         con_add_wrench(wrow, G.ext[k], es, G.pose[k], SV<T>{V3<T>{lam[0], lam[1], lam[2]}, V3<T>{lam[3], lam[4], lam[5]}});
         if constexpr (REL)
            if (G.base[k] >= 0)
            { // the opposite wrench at the same point, on the base body
               const SV<T> fb = force_to_parent(con_load_pose(G.zpose + 12L * k * B + cfg, B), SV<T>{V3<T>{lam[0], lam[1], lam[2]}, V3<T>{lam[3], lam[4], lam[5]}});
               T *ob = wrow + (long)G.bext[k] * 6 * es;
               ob[0] -= fb.a.x, ob[es] -= fb.a.y, ob[2 * es] -= fb.a.z, ob[3 * es] -= fb.l.x, ob[4 * es] -= fb.l.y, ob[5 * es] -= fb.l.z;
            }
      }
   }
}

// out += x, elementwise: qd_out = qd + H^-1 J^T Lambda of mh_constraint_impulse_* (one layout for both: plain index)
template <typename T>
__global__ void __launch_bounds__(256) add_in_place_kernel(T *out, const T *x, long n)
{
   const long stride = (long)gridDim.x * blockDim.x;
   for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
      out[i] += x[i];
}
} // namespace mh
