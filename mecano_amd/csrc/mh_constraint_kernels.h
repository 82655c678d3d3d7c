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
   const T *q;          // acceleration form only (the root acceleration is brought to the bodies)
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

template <typename T>
__global__ void __launch_bounds__(64) constraint_solve_kernel(ConArgs<T> G)
{
   const DevModel &m = G.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map);
   const long nlanes = (long)gridDim.x * blockDim.x;
   const long B = G.B, ld = 6L * G.K;
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
         if (!G.velocity)
         {
            const XF<T> Xb = body_pose_in_root<T>(m, meta, cfg_map, CB, G.q + cfg * G.q_bs, G.q_es, G.tgt[k]);
            v = v - motion_to_child(Xb, root_acceleration(G));
         }
         const T *ps = G.pose[k];
         const XF<T> Xt{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
         v = motion_to_child(Xt, v);
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
         const T *ps = G.pose[k];
         const XF<T> Xt{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
         const SV<T> f = force_to_parent(Xt, SV<T>{V3<T>{lam[0], lam[1], lam[2]}, V3<T>{lam[3], lam[4], lam[5]}});
         T *o = wrow + (long)G.ext[k] * 6 * G.f_es; // (two targets on one body: the lane reads back its own store)
         const long es = G.f_es;
         o[0] += f.a.x, o[es] += f.a.y, o[2 * es] += f.a.z, o[3 * es] += f.l.x, o[4 * es] += f.l.y, o[5 * es] += f.l.z;
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
