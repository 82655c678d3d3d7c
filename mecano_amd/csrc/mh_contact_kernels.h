// mh_contact_kernels.h -- the frictional contact solve between the two launches of mh_contact_impulse_* (run-time topology, one lane per
// configuration, gfx950).  The launches around it are those of mh_constraint_impulse_* (mh_constraint_kernels.h): per-body twists, the
// COUPLED inverse apparent inertia W = J H^-1 J^T into SoA scratch, this kernel, forward dynamics at rest with the impulses as wrenches.
//
// K contact points, the origins of K target frames.  u_k: linear velocity of frame k relative to the root body, in the target frame;
// lambda_k: impulse on the target body there; n_k = R_pose^T R_body(q)^T n^_k the unit normal brought from the root body frame into the
// target frame; mu_k the friction coefficient; v_k the least normal velocity after the impulse; eps the compliance.  Per configuration the
// unique minimiser of the cone-constrained convex problem (Anitescu's time-stepping relaxation)
//    minimise 1/2 lambda^T (S + eps I) lambda + lambda^T b   subject to  lambda_k in C_k = { n_k.lambda_k >= 0, |tangential part| <= mu_k n_k.lambda_k }
//    b_k = u_k(qd) - v_k n_k,     qd_out = qd + H^-1 J_c^T lambda.
// At mu = 0 this is the frictionless complementarity solution 0 <= n.lambda  _|_  n.u+ - v + eps n.lambda >= 0; a contact whose stick
// solution lies inside its cone sticks; a sliding contact has |lambda_t| = mu lambda_n opposed to its tangential velocity -- and, the
// relaxation's known artefact, lifts off along the normal at a speed of mu times its sliding speed.
//
// S: the linear 3 x 3 sub-blocks of W (rows / columns 6 k + 3 ... 6 k + 5).  Block (k, l) with l < k as read, its transpose for (l, k), the
// lower triangle of a diagonal block mirrored: ONE exactly symmetric quadratic form (W is symmetric up to rounding only).
//   0. + 1. (rolled over k) one climb per target (body_pose_in_root), n_k and b_k from the twists the first launch wrote, both parked in
//      the scratch behind W ([3 K][B] each).
//   2. lambda (3 K values), n_k, rho_k = 1 / (trace S_kk + eps) and the activity bits in registers: every loop over contacts below is
//      unrolled to KMAX with uniform guards, so that no index into them is a run-time one.  lambda^0 = Pi_k(linear rows of impulse_init)
//      or 0.  Then n_iterations projected block Gauss-Seidel sweeps, k = 0 ... K - 1 in list order with the newest lambda:
//         u = b_k + sum_l S_kl lambda_l + eps lambda_k;   lambda_k = Pi_k(lambda_k - rho_k u)
//      rho_k <= 1 / lambda_max(S_kk + eps I): each block step descends the objective.  Pi_k is the Euclidean projection onto C_k: with
//      s = n.x, t = x - s n, r = |t|:  x if r <= mu s;  0 if mu r <= -s;  else s' n + (mu s' / r) t with s' = (s + mu r) / (1 + mu^2).  The
//      map is nonexpansive and has no discontinuous branch.  An inactive contact keeps lambda = 0 exactly (its terms add exact zeros and
//      its update is discarded); nothing else depends on the lane.
//      RESIDENT: the lower block triangle of S, 9 K (K + 1) / 2 entries per lane, is copied once into LDS laid out [entry][lane] -- 8-byte
//      reads of 32 consecutive lanes cover the 64 banks once, 4-byte reads the 32 -- and the sweeps read it there; otherwise they read W in
//      the SoA scratch, contiguous across lanes.  Both forms fetch the same numbers and run the same operations in the same order
//      (contact_plan in mh_launch_plans.h chooses).
//   3. impulse_out (rows 0-2 and every row of an inactive contact exactly 0), residual_out (largest |change of a component| in the last
//      sweep), and the complete wrench matrix of the second launch: zeros plus X_k^T (0, lambda_k).
// A configuration gets quiet NaN in all its outputs when trace S_kk + eps of an active contact is not positive and finite, the norm
// of its n^ is not positive and finite, its b_k is not finite or an impulse after the last sweep is not finite; the tests read bits
// (pivot_ok, contact_finite): the translation unit is compiled with -ffinite-math-only.
//
// REL = true: mh_contact_impulse_between_*, where contact k acts between the target body and the body of base[k] (the root where
// base[k] < 0, with the arithmetic above).  Four more instantiations per precision: the rooted ones keep their code.
//   0. a contact with a non-root base: Z_k, the pose of target frame k in the body-fixed frame of its base, from two climbs
//      (body_pose_in_root, con_relative), parked in scratch ([12 K][B]); b_k = linear rows of (X_k v_t - Z_k v_b) - v_k n_k.  n^_k points
//      from the base body into the target body and is still given in the root body frame: n_k as above, from the target's climb.
//   1. W arrives for n_app = K + (non-root bases) frames and is reduced to that of the relative motions in place over the target blocks
//      (con_reduce_relative, the step the constraint kernel runs) BEFORE the sweep state is live; ld = 6 n_app from here on.  The copy
//      into LDS follows the reduction; the streamed form reads the reduced W: the same bits either way.
//   3. the base body receives -Z_k^T (0, lambda_k).
#pragma once
#include "mh_constraint_kernels.h"

namespace mh
{
constexpr int CONTACT_MAX_TARGETS = 8; // MH_MAX_CONTACT_TARGETS

template <typename T>
struct ContactArgs
{
   DevModel m;
   long B;
   const T *q;
   long q_bs, q_es;
   const T *body;       // [B][n_joints][6] with (f_bs, f_es): per-body twists of (q, qd)
   T *wrench;           // same shape: what the second launch reads
   long f_bs, f_es;
   const T *W;          // [(6 K)^2][B]
   T *bvec, *nvec;      // [3 K][B] each: b, the normals in the target frames
   const int *active;   // [B][K] with (a_bs, a_es), or NULL = every contact closed (v_normal shares the strides)
   const T *v_normal;   // or NULL = zeros
   long a_bs, a_es;
   const T *normals;    // [B][K][3] with (n_bs, n_es), or NULL = (0, 0, 1)
   long n_bs, n_es;
   const T *init;       // [B][K][6] with (d_bs, d_es), or NULL = zeros; may be `impulse`
   T *impulse;          // same shape, or NULL
   long d_bs, d_es;
   T *residual;         // [B], or NULL
   T eps;
   int K, n_iter;
   int tgt[CONTACT_MAX_TARGETS]; // engine index of the target's body
   int ext[CONTACT_MAX_TARGETS]; // its joint in the caller's order
   T mu[CONTACT_MAX_TARGETS];    // min(mu_k, 1 / mu_k), formed in fp64 on the host
   unsigned wide;                // bit k: mu_k > 1
   T pose[CONTACT_MAX_TARGETS][12];
};

// the relative form's additions
template <typename T>
struct ContactRelArgs : ContactArgs<T>
{
   T *Wrel;                          // W again, writable: reduced in place to that of the relative motions
   T *zpose;                         // [12 K][B]: Z_k of the contacts with a non-root base
   int n_app;                        // frames of W: K targets, then the non-root bases
   int base[CONTACT_MAX_TARGETS];    // engine index of the base's body, -1 = the root body
   int bext[CONTACT_MAX_TARGETS];    // its joint in the caller's order
   int bslot[CONTACT_MAX_TARGETS];   // its frame in W (>= K), -1 = the root body
};

// Euclidean projection of x onto the cone { n.x >= 0, |x - (n.x) n| <= mu n.x }.  m = min(mu, 1 / mu), wide = mu > 1 (uniform: the host
// forms both): a wide cone is worked with a = 1 / mu -- r <= mu s as a r <= s, s' = a (a s + r) / (1 + a^2), the tangential factor
// (a s + r) / ((1 + a^2) r) -- so that no finite mu overflows (mu^2 does from 1.85e19 in fp32: s' = 0 and the origin where the
// tangential part belongs) and the limit is the projection onto the half space n.x >= 0.  Up to mu = 1 the operations are the stated ones.
template <typename T>
MH_DEV void contact_project(T &x0, T &x1, T &x2, T n0, T n1, T n2, T m, bool wide)
{
   const T s = fma(n2, x2, fma(n1, x1, n0 * x0));
   const T t0 = fma(-s, n0, x0), t1 = fma(-s, n1, x1), t2 = fma(-s, n2, x2);
   const T r = sqrt(fma(t2, t2, fma(t1, t1, t0 * t0)));
   const bool inside = wide ? m * r <= s : r <= m * s, polar = wide ? r <= -(m * s) : m * r <= -s;
   const T w = (wide ? fma(m, s, r) : fma(m, r, s)) / fma(m, m, T(1));
   const T s1 = wide ? m * w : w;
   const T c = (wide ? w : m * w) / r; // (r = 0 lands in one of the first two cases: this quotient is then discarded)
   const T y0 = fma(c, t0, s1 * n0), y1 = fma(c, t1, s1 * n1), y2 = fma(c, t2, s1 * n2);
   x0 = inside ? x0 : (polar ? T(0) : y0);
   x1 = inside ? x1 : (polar ? T(0) : y1);
   x2 = inside ? x2 : (polar ? T(0) : y2);
}

// neither infinite nor NaN, read from bits the compiler cannot trace back to a floating-point value: under -ffinite-math-only it
// recognises the mask-and-compare on the bits of an fma's result as a class test and folds it to true (seen in the code object)
MH_DEV bool contact_finite(double d)
{
   long long b = __double_as_longlong(d);
   asm volatile("" : "+v"(b));
   return (b & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}
MH_DEV bool contact_finite(float d)
{
   int b = __float_as_int(d);
   asm volatile("" : "+v"(b));
   return (b & 0x7f800000) != 0x7f800000;
}

// where entry (i, j) of S_kl lives in W (row-major with leading dimension ld = 6 K, one entry every B elements)
MH_DEV long contact_w_index(int k, int l, int i, int j, long ld)
{
   if (l < k)
      return (6L * k + 3 + i) * ld + 6L * l + 3 + j;
   if (l > k)
      return (6L * l + 3 + j) * ld + 6L * k + 3 + i;
   return (6L * k + 3 + (i > j ? i : j)) * ld + 6L * k + 3 + (i < j ? i : j);
}
// ... and in the LDS copy of the lower block triangle (diagonal blocks stored in full, mirrored)
MH_DEV constexpr int contact_lds_entry(int k, int l, int i, int j)
{
   return l <= k ? (k * (k + 1) / 2 + l) * 9 + i * 3 + j : (l * (l + 1) / 2 + k) * 9 + j * 3 + i;
}

template <typename T, bool RESIDENT, int KMAX, bool REL = false>
__global__ void __launch_bounds__(64, 2) contact_solve_kernel(std::conditional_t<REL, ContactRelArgs<T>, ContactArgs<T>> G)
{
   extern __shared__ __align__(16) unsigned char contact_lds_raw[];
   T *const sm = reinterpret_cast<T *>(contact_lds_raw) + threadIdx.x; // [entry][lane]
   const DevModel &m = G.m;
   const T *CB = (const T *)m.consts;
   const ciptr meta = as_const(m.meta), cfg_map = as_const(m.cfg_map);
   const long nlanes = (long)gridDim.x * blockDim.x;
   const int K = G.K;
   long ld = 6L * K;
   if constexpr (REL)
      ld = 6L * G.n_app;
   const long B = G.B;
   const T eps = G.eps, nan = quiet_nan(T(0));

   for (long cfg = (long)blockIdx.x * blockDim.x + threadIdx.x; cfg < B; cfg += nlanes)
   {
      const T *W = G.W + cfg;
      if constexpr (REL)
         W = G.Wrel + cfg; // (read through the pointer the reduction writes through)
      T *bv = G.bvec + cfg, *nv = G.nvec + cfg;
      const T *brow = G.body + cfg * G.f_bs;
      bool bad = false;
      // ---- 0. + 1. normals in the target frames and b
#pragma nounroll
      for (int k = 0; k < K; k++)
      {
         const bool on = G.active ? G.active[cfg * G.a_bs + k * G.a_es] != 0 : true;
         V3<T> nh{T(0), T(0), T(1)};
         if (G.normals)
         {
            const T *np = G.normals + cfg * G.n_bs + 3L * k * G.n_es;
            nh = V3<T>{np[0], np[G.n_es], np[2 * G.n_es]};
            const T nn = dot(nh, nh);
            bad = bad || (on && !pivot_ok(nn));
            nh = (T(1) / sqrt(nn)) * nh;
         }
         const T *ps = G.pose[k];
         const XF<T> Xt{M3<T>{ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8]}, V3<T>{ps[9], ps[10], ps[11]}};
         const XF<T> Xb = body_pose_in_root<T>(m, meta, cfg_map, CB, G.q + cfg * G.q_bs, G.q_es, G.tgt[k]);
         const V3<T> n = tmul(Xt.R, tmul(Xb.R, nh));
         const long e = (long)G.ext[k] * 6;
         SV<T> v = motion_to_child(Xt, SV<T>{V3<T>{brow[(e + 0) * G.f_es], brow[(e + 1) * G.f_es], brow[(e + 2) * G.f_es]},
                                             V3<T>{brow[(e + 3) * G.f_es], brow[(e + 4) * G.f_es], brow[(e + 5) * G.f_es]}});
         if constexpr (REL)
            if (G.base[k] >= 0)
            { // against a moving base: Z_k, and the base's twist brought to the target frame
               const XF<T> X_b = body_pose_in_root<T>(m, meta, cfg_map, CB, G.q + cfg * G.q_bs, G.q_es, G.base[k]);
               const XF<T> Z = con_relative(con_relative(Xb, X_b), Xt); // (the base's frame in the target body's; the target frame in the base's)
               T *z = G.zpose + 12L * k * B + cfg;
               z[0] = Z.R.xx, z[B] = Z.R.xy, z[2 * B] = Z.R.xz, z[3 * B] = Z.R.yx, z[4 * B] = Z.R.yy, z[5 * B] = Z.R.yz;
               z[6 * B] = Z.R.zx, z[7 * B] = Z.R.zy, z[8 * B] = Z.R.zz, z[9 * B] = Z.p.x, z[10 * B] = Z.p.y, z[11 * B] = Z.p.z;
               const long eb = (long)G.bext[k] * 6;
               v = v - motion_to_child(Z, SV<T>{V3<T>{brow[(eb + 0) * G.f_es], brow[(eb + 1) * G.f_es], brow[(eb + 2) * G.f_es]},
                                                V3<T>{brow[(eb + 3) * G.f_es], brow[(eb + 4) * G.f_es], brow[(eb + 5) * G.f_es]}});
            }
         const T vk = G.v_normal ? G.v_normal[cfg * G.a_bs + k * G.a_es] : T(0);
         nv[(3L * k + 0) * B] = n.x, nv[(3L * k + 1) * B] = n.y, nv[(3L * k + 2) * B] = n.z;
         const T b0 = fma(-vk, n.x, v.l.x), b1 = fma(-vk, n.y, v.l.y), b2 = fma(-vk, n.z, v.l.z);
         bad = bad || (on && !(contact_finite(b0) && contact_finite(b1) && contact_finite(b2)));
         bv[(3L * k + 0) * B] = b0, bv[(3L * k + 1) * B] = b1, bv[(3L * k + 2) * B] = b2;
      }
      if constexpr (REL) // ---- 1. W of the relative motions, in place over the targets' blocks, before the sweep state is live
         con_reduce_relative(G.Wrel + cfg, G.zpose + cfg, B, ld, K, G.bslot);
      if constexpr (RESIDENT)
      { // the lower block triangle of S into LDS (one wave per workgroup: the lane's own column, no barrier)
         for (int k = 0; k < K; k++)
            for (int l = 0; l <= k; l++)
#pragma unroll
               for (int ij = 0; ij < 9; ij++)
                  sm[((k * (k + 1) / 2 + l) * 9 + ij) * 64] = W[contact_w_index(k, l, ij / 3, ij % 3, ld) * B];
      }
      // (streamed: the stride is made opaque per block, or the 9 K^2 scalar offsets of a sweep are hoisted out of the iteration loop, spilled
      // and the lanes' registers with them -- 3.4 KB of scratch per lane at K = 8)
      auto S = [&](int k, int l, int i, int j, long stride) -> T {
         if constexpr (RESIDENT)
            return sm[contact_lds_entry(k, l, i, j) * 64];
         else
            return W[contact_w_index(k, l, i, j, ld) * stride];
      };
      // ---- 2. the state of the sweeps, in registers
      T lam[3 * KMAX], nk[3 * KMAX], rho[KMAX];
      bool act[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; k++)
      {
         lam[3 * k] = lam[3 * k + 1] = lam[3 * k + 2] = T(0);
         nk[3 * k] = nk[3 * k + 1] = nk[3 * k + 2] = T(0);
         rho[k] = T(0), act[k] = false;
         if (k < K)
         {
            act[k] = G.active ? G.active[cfg * G.a_bs + k * G.a_es] != 0 : true;
            nk[3 * k] = nv[(3L * k + 0) * B], nk[3 * k + 1] = nv[(3L * k + 1) * B], nk[3 * k + 2] = nv[(3L * k + 2) * B];
            const T d = S(k, k, 0, 0, B) + S(k, k, 1, 1, B) + S(k, k, 2, 2, B) + eps;
            bad = bad || (act[k] && !pivot_ok(d));
            rho[k] = T(1) / d;
            if (G.init && act[k])
            {
               const T *ip = G.init + cfg * G.d_bs + (6L * k + 3) * G.d_es;
               T x0 = ip[0], x1 = ip[G.d_es], x2 = ip[2 * G.d_es];
               contact_project(x0, x1, x2, nk[3 * k], nk[3 * k + 1], nk[3 * k + 2], G.mu[k], (G.wide >> k & 1u) != 0);
               lam[3 * k] = x0, lam[3 * k + 1] = x1, lam[3 * k + 2] = x2;
            }
         }
      }
      T res = T(0);
      for (int it = 0; it < G.n_iter; it++)
      {
         res = T(0);
#pragma unroll
         for (int k = 0; k < KMAX; k++)
            if (k < K)
            {
               T u0 = bv[(3L * k + 0) * B], u1 = bv[(3L * k + 1) * B], u2 = bv[(3L * k + 2) * B];
#pragma unroll
               for (int l = 0; l < KMAX; l++)
                  if (l < K)
                  {
                     const T a = lam[3 * l], b = lam[3 * l + 1], c = lam[3 * l + 2];
                     long sB = B;
                     if constexpr (!RESIDENT)
                        asm volatile("" : "+s"(sB));
                     u0 = fma(S(k, l, 0, 2, sB), c, fma(S(k, l, 0, 1, sB), b, fma(S(k, l, 0, 0, sB), a, u0)));
                     u1 = fma(S(k, l, 1, 2, sB), c, fma(S(k, l, 1, 1, sB), b, fma(S(k, l, 1, 0, sB), a, u1)));
                     u2 = fma(S(k, l, 2, 2, sB), c, fma(S(k, l, 2, 1, sB), b, fma(S(k, l, 2, 0, sB), a, u2)));
                  }
               u0 = fma(eps, lam[3 * k], u0), u1 = fma(eps, lam[3 * k + 1], u1), u2 = fma(eps, lam[3 * k + 2], u2);
               T x0 = fma(-rho[k], u0, lam[3 * k]), x1 = fma(-rho[k], u1, lam[3 * k + 1]), x2 = fma(-rho[k], u2, lam[3 * k + 2]);
               contact_project(x0, x1, x2, nk[3 * k], nk[3 * k + 1], nk[3 * k + 2], G.mu[k], (G.wide >> k & 1u) != 0);
               x0 = act[k] ? x0 : T(0), x1 = act[k] ? x1 : T(0), x2 = act[k] ? x2 : T(0);
               res = fmax(res, fmax(fabs(x0 - lam[3 * k]), fmax(fabs(x1 - lam[3 * k + 1]), fabs(x2 - lam[3 * k + 2]))));
               lam[3 * k] = x0, lam[3 * k + 1] = x1, lam[3 * k + 2] = x2;
            }
      }
      // a sweep state that is no number (a NaN in qd, in v_normal or in impulse_init of a closed contact; an overflow) would leave fmax
      // with the last finite change in res: such a configuration reads as converged.  It is bad like the others
#pragma unroll
      for (int k = 0; k < KMAX; k++)
         if (k < K)
            bad = bad || !(contact_finite(lam[3 * k]) && contact_finite(lam[3 * k + 1]) && contact_finite(lam[3 * k + 2]));
      // ---- 3. impulse_out, residual_out and the wrenches of the second launch
      if (G.residual)
         G.residual[cfg] = bad ? nan : res;
      T *wrow = G.wrench + cfg * G.f_bs;
      for (long e = 0; e < 6L * m.n; e++)
         wrow[e * G.f_es] = bad ? nan : T(0);
#pragma unroll
      for (int k = 0; k < KMAX; k++)
         if (k < K)
         {
            const T z = bad ? nan : T(0);
            const T f0 = bad ? nan : lam[3 * k], f1 = bad ? nan : lam[3 * k + 1], f2 = bad ? nan : lam[3 * k + 2];
            if (G.impulse)
            {
               T *op = G.impulse + cfg * G.d_bs + 6L * k * G.d_es;
               op[0] = z, op[G.d_es] = z, op[2 * G.d_es] = z, op[3 * G.d_es] = f0, op[4 * G.d_es] = f1, op[5 * G.d_es] = f2;
            }
            con_add_wrench(wrow, G.ext[k], G.f_es, G.pose[k], SV<T>{V3<T>{z, z, z}, V3<T>{f0, f1, f2}});
            if constexpr (REL)
               if (G.base[k] >= 0)
               { // the opposite impulse at the same point, on the base body
                  const long es = G.f_es;
                  const SV<T> fb = force_to_parent(con_load_pose(G.zpose + 12L * k * B + cfg, B), SV<T>{V3<T>{z, z, z}, V3<T>{f0, f1, f2}});
                  T *ob = wrow + (long)G.bext[k] * 6 * es;
                  ob[0] -= fb.a.x, ob[es] -= fb.a.y, ob[2 * es] -= fb.a.z, ob[3 * es] -= fb.l.x, ob[4 * es] -= fb.l.y, ob[5 * es] -= fb.l.z;
               }
         }
   }
}
} // namespace mh
