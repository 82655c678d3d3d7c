// mh_limit_kernels.h -- the joint-limit solve behind the listed-column launch of mh_joint_limit_impulse_* (one lane per configuration,
// one wave per workgroup, persistent over groups of 64 configurations, gfx950).  The launch in front of it is mass_matrix_inverse_kernel
// (mh_minv_kernels.h) with the DoFs of the L listed joints as its columns, written to SoA scratch as Hinv[(r L + k) B + cfg]: row r of
// column k.  Nothing else is launched: the change of velocity is a combination of those same columns.
//
// Per configuration and row i (DoF index d_i, configuration index c_i, resolved on the host): gap_lo = q[c_i] - lower_i,
// gap_hi = upper_i - q[c_i], s_i = +1 where gap_lo <= gap_hi else -1, gap_i = the smaller; the row is CLOSED where gap_i <= margin;
// b_i = s_i qd[d_i] + erp gap_i;  S_ij = s_i s_j Hinv[d_i][d_j] read from ONE triangle (j < i: row d_i of column j; the diagonal from
// column i; j > i: S_ji), so that S is exactly symmetric.  The iterate of
//    minimise 1/2 lambda^T (S + eps I) lambda + lambda^T b   subject to  lambda >= 0  (closed rows; open rows keep 0.0 exactly)
// from lambda^0 = max(0, s_i impulse_init_i) by n_iter projected Gauss-Seidel sweeps in list order with the newest lambda:
//    u = b_i + sum_j S_ij lambda_j + eps lambda_i,    lambda_i = max(0, lambda_i - rho_i u),   rho_i = 1 / (S_ii + eps).
// The kernel keeps the SIGNED quantities t_i = s_i lambda_i (the generalised impulse on the joint, what impulse_out returns) and
// c_i = s_i b_i = qd[d_i] + s_i erp gap_i:  s_i u = c_i + sum_j Hinv_ij t_j + eps t_i, t_i <- t_i - rho_i (s_i u) clamped to the side of
// s_i.  Multiplying by +-1 is exact and rounding is symmetric under negation: these are the bits of the unsigned form, and the stored
// triangle carries no sign -- the same numbers serve every lane whatever its sides.
//   state per lane: closed and side bits of its rows in two 64-bit masks (registers); t, c and rho in LDS as [entry][lane] (3 L entries):
//      a run-time row index never addresses a register array.  RESIDENT: the lower triangle of Hinv's listed block, L (L + 1) / 2 entries
//      per lane, behind them, gathered once; otherwise the sweeps stream those entries from the columns, the loads of eight entries of a
//      row issued ahead of the multiply-adds that wait for them.  Both forms fetch the same numbers and run the same operations in the
//      same order (limit_plan in mh_launch_plans.h chooses by capacity).
//   a row no lane of the wave has closed (ballot) is skipped by one wave-uniform branch, as a row of the sweep and as a column of every sum:
//      its t is zero in every lane.  A lane whose row is open beside a neighbour's closed one discards its update.
//   outputs: qd_out[r] = qd[r] + sum over the lane's closed rows, in list order, of t_i Hinv[r][i] (no closed row: the bits of qd; entries
//      no joint owns: Hinv's row is zero and the sum adds nothing); impulse_out = t; residual_out = largest |change of a t_i| in the last sweep.
//      SoA stores are contiguous across lanes.  AoS rows are written by direct stores, one entry per lane and instruction: a
//      configuration's row is nv entries against the nv L entries of Hinv the lane reads for it, and staging the rows through LDS would
//      take nv entries per lane from the budget that decides whether S is resident.
// A configuration gets quiet NaN in all three outputs when q[c_i] of a listed joint is not finite, S_ii + eps of a closed row is not
// positive and finite, b_i of a closed row or impulse_init_i of a closed row is not finite, or a t after the last sweep is not finite;
// the tests read bits (pivot_ok, contact_finite): the translation unit is compiled with -ffinite-math-only.
#pragma once
#include "mh_contact_kernels.h"

namespace mh
{
constexpr int LIMIT_MAX_JOINTS = 64; // MH_MAX_LIMIT_JOINTS = MINV_MAX_COLUMNS
constexpr int LIMIT_AHEAD = 8;       // entries of Hinv whose loads are in flight together

template <typename T>
struct LimitArgs
{
   long B;
   int nv, L, n_iter;
   const T *q;
   long q_bs, q_es;
   const T *qd;
   T *out; // qd_out, the strides of qd
   long v_bs, v_es;
   const T *Hinv;    // [nv L][B]
   const T *init;    // [B][L] with (d_bs, d_es), or NULL = zeros; may be `impulse`
   T *impulse;       // same shape, or NULL
   long d_bs, d_es;
   T *residual;      // [B], or NULL
   T eps, margin, erp;
   int dof[LIMIT_MAX_JOINTS], cfg[LIMIT_MAX_JOINTS]; // d_i, c_i
   T lower[LIMIT_MAX_JOINTS], upper[LIMIT_MAX_JOINTS];
};

// where entry (i, j) of the symmetrised listed block lives in the LDS triangle, behind the 3 L state entries
MH_DEV int limit_lds_entry(int i, int j, int L)
{
   const int hi = i > j ? i : j, lo = i > j ? j : i;
   return 3 * L + hi * (hi + 1) / 2 + lo;
}
// ... and in Hinv (one entry every B elements)
MH_DEV long limit_h_index(int i, int j, const int *dof, int L)
{
   const int hi = i > j ? i : j, lo = i > j ? j : i;
   return (long)dof[hi] * L + lo;
}

template <typename T, bool RESIDENT>
__global__ void __launch_bounds__(64) limit_solve_kernel(LimitArgs<T> G)
{
   extern __shared__ __align__(16) unsigned char limit_lds_raw[];
   T *const sm = reinterpret_cast<T *>(limit_lds_raw) + threadIdx.x; // [entry][lane]: t at i, c at L + i, rho at 2 L + i, then the triangle
   const int L = G.L, nv = G.nv;
   const long B = G.B;
   const T eps = G.eps, nan = quiet_nan(T(0));
   typedef unsigned long long mask_t;

   for (long first = (long)blockIdx.x * 64; first < B; first += (long)gridDim.x * 64)
   {
      const bool valid = first + threadIdx.x < B;
      const long cfg = valid ? first + threadIdx.x : B - 1; // a lane beyond the batch reads the last configuration and writes nothing
      const T *H = G.Hinv + cfg;
      const T *qrow = G.q + cfg * G.q_bs, *vrow = G.qd + cfg * G.v_bs;
      mask_t closed = 0, side = 0, wave = 0; // bit i: row i is closed in this lane; its side is the lower limit; closed in some lane of the wave
      bool bad = false;
      // ---- rows, sides, gaps, c, rho and the start
      for (int i = 0; i < L; i++)
      {
         const T qv = qrow[G.cfg[i] * G.q_es];
         const T gap_lo = qv - G.lower[i], gap_hi = G.upper[i] - qv;
         const bool low = gap_lo <= gap_hi;
         const T gap = low ? gap_lo : gap_hi;
         const bool on = valid && gap <= G.margin;
         bad = bad || !contact_finite(qv);
         const T c = fma(low ? G.erp : -G.erp, gap, vrow[G.dof[i] * G.v_es]);
         const T d = H[limit_h_index(i, i, G.dof, L) * B] + eps;
         T t = T(0);
         if (G.init && on)
         {
            t = G.init[cfg * G.d_bs + i * G.d_es];
            bad = bad || !contact_finite(t);
            t = low ? fmax(t, T(0)) : fmin(t, T(0));
         }
         bad = bad || (on && !(contact_finite(c) && pivot_ok(d)));
         sm[i * 64] = t, sm[(L + i) * 64] = c, sm[(2 * L + i) * 64] = T(1) / d;
         closed |= on ? (mask_t)1 << i : 0, side |= low ? (mask_t)1 << i : 0;
         wave |= __ballot(on) != 0 ? (mask_t)1 << i : 0;
      }
      // `wave` is made a scalar: the rows and columns below are walked bit by bit on the scalar unit.  readfirstlane returns an int: each
      // half goes through unsigned before it is widened, or a closed row 31 would set bits 32 ... 63 and the walks would take rows past L
      wave = (mask_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(wave >> 32)) << 32 |
             (mask_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)wave);
      if constexpr (RESIDENT)
      { // the lower triangle of the listed block into LDS, the entries the sweeps read: rows and columns closed in some lane (one wave per
        // workgroup: the lane's own column, no barrier)
         for (mask_t rows = wave; rows; rows &= rows - 1)
         {
            const int i = __builtin_ctzll(rows);
            for (mask_t cols = wave & (((mask_t)2 << i) - 1); cols; cols &= cols - 1)
            {
               const int j = __builtin_ctzll(cols);
               sm[limit_lds_entry(i, j, L) * 64] = H[limit_h_index(i, j, G.dof, L) * B];
            }
         }
      }
      // ---- the sweeps
      T res = T(0);
      for (int it = 0; it < G.n_iter; it++)
      {
         res = T(0);
         for (mask_t rows = wave; rows; rows &= rows - 1)
         {
            const int i = __builtin_ctzll(rows);
            T acc = sm[(L + i) * 64];
            for (mask_t cols = wave; cols;)
            { // the next LIMIT_AHEAD closed columns: every load issued, then the multiply-adds in list order
               int j[LIMIT_AHEAD];
               bool use[LIMIT_AHEAD];
               T h[LIMIT_AHEAD];
#pragma unroll
               for (int k = 0; k < LIMIT_AHEAD; k++)
               {
                  use[k] = cols != 0;
                  j[k] = use[k] ? __builtin_ctzll(cols) : i; // (an idle slot reads the diagonal again and discards it)
                  cols &= cols - 1;
                  if constexpr (RESIDENT)
                     h[k] = sm[limit_lds_entry(i, j[k], L) * 64];
                  else
                     h[k] = H[limit_h_index(i, j[k], G.dof, L) * B];
               }
#pragma unroll
               for (int k = 0; k < LIMIT_AHEAD; k++)
                  acc = use[k] ? fma(h[k], sm[j[k] * 64], acc) : acc;
            }
            const T t = sm[i * 64];
            const T x = fma(-sm[(2 * L + i) * 64], fma(eps, t, acc), t);
            T y = (side >> i) & 1 ? fmax(x, T(0)) : fmin(x, T(0));
            y = (closed >> i) & 1 ? y : T(0);
            res = fmax(res, fabs(y - t));
            sm[i * 64] = y;
         }
      }
      // a sweep state that is no number would leave fmax with the last finite change in res: such a configuration is bad like the others
      for (int i = 0; i < L; i++)
         bad = bad || !contact_finite(sm[i * 64]);
      // ---- outputs
      if (valid)
      {
         if (G.residual)
            G.residual[cfg] = bad ? nan : res;
         if (G.impulse)
            for (int i = 0; i < L; i++)
               G.impulse[cfg * G.d_bs + i * G.d_es] = bad ? nan : ((closed >> i) & 1 ? sm[i * 64] : T(0));
      }
      T *orow = G.out + cfg * G.v_bs;
      for (int r = 0; r < nv; r++)
      {
         T acc = vrow[r * G.v_es];
         const T *Hr = H + (long)r * L * B;
         for (mask_t cols = wave; cols;)
         {
            int i[LIMIT_AHEAD];
            bool use[LIMIT_AHEAD];
            T h[LIMIT_AHEAD];
#pragma unroll
            for (int k = 0; k < LIMIT_AHEAD; k++)
            {
               use[k] = cols != 0;
               i[k] = use[k] ? __builtin_ctzll(cols) : 0;
               cols &= cols - 1;
               h[k] = Hr[i[k] * B];
            }
#pragma unroll
            for (int k = 0; k < LIMIT_AHEAD; k++)
               acc = use[k] && ((closed >> i[k]) & 1) ? fma(sm[i[k] * 64], h[k], acc) : acc;
         }
         if (valid)
            orow[r * G.v_es] = bad ? nan : acc;
      }
   }
}
} // namespace mh
