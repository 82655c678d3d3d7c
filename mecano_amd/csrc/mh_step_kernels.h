// mh_step_kernels.h -- the chart of the velocity-space derivatives and the linearisation of the simulation step.
//
//   configuration_add_kernel         q_out = q (+) dq: MultiBodySystemStateIntegrator.integrateFromVelocity with dt = 1 and twist dq
//                                    (tools/MultiBodySystemStateIntegrator.java:164-243), per joint
//   configuration_difference_kernel  the dq with q0 (+) dq = q1, rotations in their shortest form
//   step_assemble_aos_kernel /       A [2nv][2nv] and B [2nv][nv] of x' = (q_next, qd_next) of "forward dynamics, then integrate_joint with
//   step_assemble_soa_kernel         step dt" from d qdd / d q, d qdd / d qd and H^-1 (mh_aba_derivatives_*)
//   integrate_vjp_aos_kernel /       the transpose of integrate_joint's tangent map applied to cotangents of (dq', dqd'): gq, gqd, gqdd
//   integrate_vjp_soa_kernel         (mh_integrate_vjp_*, and the integrator's share of mh_aba_integrate_vjp_*)
//   integrate_jvp_aos_kernel /       integrate_joint's tangent map applied to directions (dq, dqd, dqdd): dq', dqd'
//   integrate_jvp_soa_kernel         (mh_integrate_jvp_*, and the last launch of mh_aba_integrate_jvp_*)
//
// The step of one joint, in joint-local components (pose (R, p), twist (w, v), acceleration (al, a) from forward dynamics; integrate_sixdof):
//   a_o = a + w x v,  r = dt w + dt^2/2 al,  E = exp(r),  d = dt v + dt^2/2 a_o,  c = v + dt a_o
//   R' = R E,  p' = p + R d,  w' = w + dt al,  v' = E^T c
// and its first-order perturbation, every increment in the frame after the joint (dth, dp: the (+) chart; J_r: right Jacobian of SO(3)):
//   dr   = dt dw + dt^2/2 dal
//   dth' = E^T dth + J_r dr
//   da_o = da + dw x v + w x dv
//   dp'  = E^T (dp + dth x d + dt dv + dt^2/2 da_o)
//   dw'  = dw + dt dal
//   dv'  = v' x (J_r dr) + E^T (dv + dt da_o)
// R and p do not appear.  A spherical joint is the rotational half, a planar joint the restriction to the XZ plane (rotation vector along
// y, where J_r dr = dr), a 1-DoF joint dq' = dq + dt dqd + dt^2/2 dqdd, dqd' = dqd + dt dqdd.  Column c of the row block of a joint is this
// map applied to (dq, dqd) = the joint's own unit increment where c is one of its columns, and dqdd = the joint's rows of column c of
// [d qdd / d q | d qdd / d qd | H^-1]: every element of those three matrices is read once, every element of A and B written once.
//
// AoS: a workgroup per configuration; the joints' small matrices (E, J_r, d, v, w, v') are formed once per configuration by one thread per
// joint and shared through LDS; the threads then run along the COLUMNS of the three inputs, so that every global load of a row and every
// store of a row of A and B is contiguous across lanes.  Nothing of size nv^2 is staged: rows stream, whatever nv is.
// SoA: lanes run along the batch, the joint's small matrices stay in registers.
#pragma once
#include "mh_kernels.h"

namespace mh
{
// ---- exp and right Jacobian of SO(3) from the rotation vector r: E = I + a K + b K^2, J_r = I - b K + c K^2, K = [r]x,
//      a = sin th / th, b = (1 - cos th) / th^2 (as 2 sin^2(th/2) / th^2: no cancellation), c = (th - sin th) / th^3 (series below
//      th = 1/4, where the closed form cancels).  Below the step's own threshold |r| = 1e-12 E is the identity, as in integrate_sixdof.
template <typename T>
MH_DEV void so3_exp_jr(V3<T> r, M3<T> &E, M3<T> &Jr)
{
   const T t2 = dot(r, r), th = sqrt(t2);
   T a = T(0), b = T(0), bj = T(0.5), c = T(1) / T(6);
   if (th >= T(1.0e-12))
   {
      T sh, ch;
      sincos_t(T(0.5) * th, sh, ch);
      const T s = T(2) * sh * ch, si = sh / th;
      a = s / th;
      b = bj = T(2) * si * si;
      if (th < T(0.25))
         c = T(1) / T(6) - t2 * (T(1) / T(120) - t2 * (T(1) / T(5040) - t2 * (T(1) / T(362880) - t2 * (T(1) / T(39916800) - t2 * (T(1) / T(6227020800.0))))));
      else
         c = (th - s) / (t2 * th);
   }
   // K^2 = r r^T - th^2 I
   const T xx = -(r.y * r.y + r.z * r.z), yy = -(r.x * r.x + r.z * r.z), zz = -(r.x * r.x + r.y * r.y);
   const T xy = r.x * r.y, xz = r.x * r.z, yz = r.y * r.z;
   E.xx = T(1) + b * xx, E.xy = b * xy - a * r.z, E.xz = b * xz + a * r.y;
   E.yx = b * xy + a * r.z, E.yy = T(1) + b * yy, E.yz = b * yz - a * r.x;
   E.zx = b * xz - a * r.y, E.zy = b * yz + a * r.x, E.zz = T(1) + b * zz;
   Jr.xx = T(1) + c * xx, Jr.xy = c * xy + bj * r.z, Jr.xz = c * xz - bj * r.y;
   Jr.yx = c * xy - bj * r.z, Jr.yy = T(1) + c * yy, Jr.yz = c * yz + bj * r.x;
   Jr.zx = c * xz + bj * r.y, Jr.zy = c * yz - bj * r.x, Jr.zz = T(1) + c * zz;
}

// what the perturbation of one joint's step needs of its state
template <typename T>
struct StepLin
{
   M3<T> E, Jr;
   V3<T> d, v, w, vn;
};
template <typename T>
MH_DEV void step_lin(T dt, T hdd, V3<T> w, V3<T> v, V3<T> al, V3<T> a, StepLin<T> &L)
{
   const V3<T> a_o = a + cross(w, v);
   so3_exp_jr<T>(dt * w + hdd * al, L.E, L.Jr);
   L.d = dt * v + hdd * a_o;
   L.v = v, L.w = w;
   L.vn = tmul(L.E, v + dt * a_o);
}
template <typename T>
MH_DEV void step_apply(const StepLin<T> &L, T dt, T hdd, V3<T> dth, V3<T> dp, V3<T> dw, V3<T> dv, V3<T> dal, V3<T> da, V3<T> &oth, V3<T> &op,
                       V3<T> &ow, V3<T> &ov)
{
   const V3<T> jr = mul(L.Jr, dt * dw + hdd * dal);
   const V3<T> dao = da + cross(dw, L.v) + cross(L.w, dv);
   oth = tmul(L.E, dth) + jr;
   op = tmul(L.E, dp + cross(dth, L.d) + dt * dv + hdd * dao);
   ow = dw + dt * dal;
   ov = cross(L.vn, jr) + tmul(L.E, dv + dt * dao);
}
// One joint, one column: x = the joint's rows of the column of d qdd / d(.), eq / ev = the joint's own unit increments of dq / dqd in that
// column (0 or 1), all in the joint's DoF order; oq / ov = the joint's rows of dq' / dqd'.  Entries beyond the joint's DoFs are not read.
template <typename T>
MH_DEV void step_column(int type, const StepLin<T> &L, T dt, T hdd, const T (&x)[6], const T (&eq)[6], const T (&ev)[6], T (&oq)[6], T (&ov)[6])
{
   const V3<T> z{T(0), T(0), T(0)};
   V3<T> o0, o1, o2, o3;
   if (type == JT_SIXDOF)
   {
      step_apply<T>(L, dt, hdd, V3<T>{eq[0], eq[1], eq[2]}, V3<T>{eq[3], eq[4], eq[5]}, V3<T>{ev[0], ev[1], ev[2]}, V3<T>{ev[3], ev[4], ev[5]},
                    V3<T>{x[0], x[1], x[2]}, V3<T>{x[3], x[4], x[5]}, o0, o1, o2, o3);
      oq[0] = o0.x, oq[1] = o0.y, oq[2] = o0.z, oq[3] = o1.x, oq[4] = o1.y, oq[5] = o1.z;
      ov[0] = o2.x, ov[1] = o2.y, ov[2] = o2.z, ov[3] = o3.x, ov[4] = o3.y, ov[5] = o3.z;
   }
   else if (type == JT_SPHERICAL)
   {
      step_apply<T>(L, dt, hdd, V3<T>{eq[0], eq[1], eq[2]}, z, V3<T>{ev[0], ev[1], ev[2]}, z, V3<T>{x[0], x[1], x[2]}, z, o0, o1, o2, o3);
      oq[0] = o0.x, oq[1] = o0.y, oq[2] = o0.z;
      ov[0] = o2.x, ov[1] = o2.y, ov[2] = o2.z;
   }
   else if (type == JT_PLANAR)
   { // (w_y, v_x, v_z): the 6-DoF map on the XZ plane, which it leaves invariant
      step_apply<T>(L, dt, hdd, V3<T>{T(0), eq[0], T(0)}, V3<T>{eq[1], T(0), eq[2]}, V3<T>{T(0), ev[0], T(0)}, V3<T>{ev[1], T(0), ev[2]},
                    V3<T>{T(0), x[0], T(0)}, V3<T>{x[1], T(0), x[2]}, o0, o1, o2, o3);
      oq[0] = o0.y, oq[1] = o1.x, oq[2] = o1.z;
      ov[0] = o2.y, ov[1] = o3.x, ov[2] = o3.z;
   }
   else
   { // revolute, prismatic
      oq[0] = eq[0] + dt * ev[0] + hdd * x[0];
      ov[0] = ev[0] + dt * x[0];
   }
}
// the joint's state, in the 6-DoF form of step_lin, from rows of qd and qdd (element stride es)
template <typename T, class IP>
MH_DEV void step_lin_of_joint(int type, IP di, const T *vr, const T *ar, long es, T dt, T hdd, StepLin<T> &L)
{
   const V3<T> z{T(0), T(0), T(0)};
   if (type == JT_SIXDOF)
      step_lin<T>(dt, hdd, V3<T>{vr[di[0] * es], vr[di[1] * es], vr[di[2] * es]}, V3<T>{vr[di[3] * es], vr[di[4] * es], vr[di[5] * es]},
                  V3<T>{ar[di[0] * es], ar[di[1] * es], ar[di[2] * es]}, V3<T>{ar[di[3] * es], ar[di[4] * es], ar[di[5] * es]}, L);
   else if (type == JT_SPHERICAL)
      step_lin<T>(dt, hdd, V3<T>{vr[di[0] * es], vr[di[1] * es], vr[di[2] * es]}, z, V3<T>{ar[di[0] * es], ar[di[1] * es], ar[di[2] * es]}, z, L);
   else if (type == JT_PLANAR)
      step_lin<T>(dt, hdd, V3<T>{T(0), vr[di[0] * es], T(0)}, V3<T>{vr[di[1] * es], T(0), vr[di[2] * es]}, V3<T>{T(0), ar[di[0] * es], T(0)},
                  V3<T>{ar[di[1] * es], T(0), ar[di[2] * es]}, L);
}

template <typename T>
struct StepArgs
{
   DevModel m;
   long B;
   T dt;
   const T *qd, *qdd;        // [B][nv] in the call's layout (v_bs, v_es)
   const T *Dq, *Dv, *Hinv;  // [B][nv][nv] (d_bs, d_es)
   T *A, *Bm;                // [B][2nv][2nv] (a_bs, a_es), [B][2nv][nv] (b_bs, b_es); either may be NULL
   const int *unowned;       // DoF indices no joint owns
   int n_unowned;
   long v_bs, v_es, d_bs, d_es, a_bs, a_es, b_bs, b_es;
};
constexpr int STEP_JOINTS = 64; // joints whose small matrices share LDS at a time
template <typename T>
struct StepJoint
{
   StepLin<T> L;
   int type, k, dof[6];
};
// rows dof (dq') and nv + dof (dqd') of A and B for column c of [Dq | Dv | Hinv] (0 <= c < 3 nv), one joint
template <typename T>
MH_DEV void step_item(const StepArgs<T> &S, long cfg, int type, int k, const int *dof, const StepLin<T> &L, int c, T dt, T hdd)
{
   const int nv = S.m.nv, seg = c < nv ? 0 : (c < 2 * nv ? 1 : 2), cc = c - seg * nv;
   if (seg == 2 ? !S.Bm : !S.A)
      return;
   const T *src = (seg == 0 ? S.Dq : (seg == 1 ? S.Dv : S.Hinv)) + cfg * S.d_bs;
   T x[6], eq[6], ev[6], oq[6], ov[6];
#pragma unroll
   for (int m = 0; m < 6; m++)
   {
      const bool on = m < k, hit = on && cc == dof[m];
      x[m] = on ? src[((long)dof[m] * nv + cc) * S.d_es] : T(0);
      eq[m] = hit && seg == 0 ? T(1) : T(0);
      ev[m] = hit && seg == 1 ? T(1) : T(0);
   }
   step_column<T>(type, L, dt, hdd, x, eq, ev, oq, ov);
   T *out = seg == 2 ? S.Bm + cfg * S.b_bs : S.A + cfg * S.a_bs;
   const long es = seg == 2 ? S.b_es : S.a_es, width = seg == 2 ? nv : 2 * nv, col = seg == 2 ? cc : c;
#pragma unroll
   for (int m = 0; m < 6; m++)
      if (m < k)
      {
         out[((long)dof[m] * width + col) * es] = oq[m];
         out[((long)(nv + dof[m]) * width + col) * es] = ov[m];
      }
}
template <typename T>
MH_DEV void step_zero_rows(const StepArgs<T> &S, long cfg, int r, int c)
{
   const int nv = S.m.nv;
   if (c < 2 * nv)
   {
      if (S.A)
         S.A[cfg * S.a_bs + ((long)r * 2 * nv + c) * S.a_es] = T(0), S.A[cfg * S.a_bs + ((long)(nv + r) * 2 * nv + c) * S.a_es] = T(0);
   }
   else if (S.Bm)
      S.Bm[cfg * S.b_bs + ((long)r * nv + c - 2 * nv) * S.b_es] = T(0), S.Bm[cfg * S.b_bs + ((long)(nv + r) * nv + c - 2 * nv) * S.b_es] = T(0);
}
template <typename T>
__global__ void __launch_bounds__(256) step_assemble_aos_kernel(StepArgs<T> S)
{
   __shared__ StepJoint<T> js[STEP_JOINTS];
   const DevModel &m = S.m;
   const int nv = m.nv, w3 = 3 * nv, t = threadIdx.x, nt = blockDim.x;
   const T dt = S.dt, hdd = T(0.5) * S.dt * S.dt;
   for (long cfg = blockIdx.x; cfg < S.B; cfg += gridDim.x)
   {
      for (int u = t; u < S.n_unowned * w3; u += nt)
         step_zero_rows<T>(S, cfg, S.unowned[u / w3], u % w3);
      for (int j0 = 0; j0 < m.n; j0 += STEP_JOINTS)
      {
         const int nj = min(STEP_JOINTS, m.n - j0);
         __syncthreads();
         if (t < nj)
         {
            const int *mi = m.meta + (j0 + t) * MI_STRIDE;
            const int type = mi[MI_TYPE], k = dof_count(type);
            const int *di = m.dof_map + mi[MI_DOF];
            StepJoint<T> &J = js[t];
            J.type = type, J.k = k;
            for (int i = 0; i < k; i++)
               J.dof[i] = di[i];
            if (general_x(type))
               step_lin_of_joint<T, const int *>(type, di, S.qd + cfg * S.v_bs, S.qdd + cfg * S.v_bs, S.v_es, dt, hdd, J.L);
         }
         __syncthreads();
         for (int u = t; u < nj * w3; u += nt)
         {
            const int jl = u / w3;
            const StepJoint<T> &J = js[jl];
            if (J.k > 0)
               step_item<T>(S, cfg, J.type, J.k, J.dof, J.L, u - jl * w3, dt, hdd);
         }
      }
   }
}
template <typename T>
__global__ void __launch_bounds__(256) step_assemble_soa_kernel(StepArgs<T> S)
{
   const DevModel &m = S.m;
   const int nv = m.nv, w3 = 3 * nv;
   const T dt = S.dt, hdd = T(0.5) * S.dt * S.dt;
   const long nlanes = (long)gridDim.x * blockDim.x;
   for (long cfg = (long)blockIdx.x * blockDim.x + threadIdx.x; cfg < S.B; cfg += nlanes)
   {
      for (int u = 0; u < S.n_unowned; u++)
         for (int c = 0; c < w3; c++)
            step_zero_rows<T>(S, cfg, S.unowned[u], c);
      for (int j = 0; j < m.n; j++)
      {
         const int *mi = m.meta + j * MI_STRIDE;
         const int type = mi[MI_TYPE], k = dof_count(type);
         if (k == 0)
            continue;
         const int *di = m.dof_map + mi[MI_DOF];
         int dof[6];
#pragma unroll
         for (int i = 0; i < 6; i++)
            dof[i] = i < k ? di[i] : 0;
         StepLin<T> L;
         if (general_x(type))
            step_lin_of_joint<T, const int *>(type, di, S.qd + cfg * S.v_bs, S.qdd + cfg * S.v_bs, S.v_es, dt, hdd, L);
         for (int c = 0; c < w3; c++)
            step_item<T>(S, cfg, type, k, dof, L, c, dt, hdd);
      }
   }
}

// ------------------------------------------------------------------------------------------------ the transpose of the step
// Reverse mode of integrate_joint: cotangents (gth', gp', gw', gv') of a joint's (dth', dp', dw', dv') give, with the E, J_r, d, v, w, v'
// of step_lin,
//   P = E gp',  V = E gv',  s = J_r^T (gth' + gv' x v'),  g_ao = dt^2/2 P + dt V
//   gq   (dth, dp) : E gth' + d x P,            P
//   gqd  (dw,  dv) : gw' + dt s + v x g_ao,     dt P + V + g_ao x w
//   gqdd (dal, da) : dt gw' + dt^2/2 s,         g_ao
// which is step_apply transposed term by term.  A spherical joint is the rotational half, a planar joint the restriction to
// (w_y, v_x, v_z) as step_column embeds it, a 1-DoF joint gq = gq', gqd = dt gq' + gqd', gqdd = dt^2/2 gq' + dt gqd'.  Neither q nor the
// joint's pose appears.  At dt = 0 E and J_r are the identity and gq = gq', gqd = gqd', gqdd = 0 come out exactly.
template <typename T>
MH_DEV void step_apply_t(const StepLin<T> &L, T dt, T hdd, V3<T> gth, V3<T> gp, V3<T> gw, V3<T> gv, V3<T> &oth, V3<T> &op, V3<T> &ow, V3<T> &ov,
                         V3<T> &oal, V3<T> &oa)
{
   const V3<T> P = mul(L.E, gp), V = mul(L.E, gv);
   const V3<T> s = tmul(L.Jr, gth + cross(gv, L.vn));
   const V3<T> gao = hdd * P + dt * V;
   oth = mul(L.E, gth) + cross(L.d, P);
   op = P;
   ow = gw + dt * s + cross(L.v, gao);
   ov = dt * P + V + cross(gao, L.w);
   oal = dt * gw + hdd * s;
   oa = gao;
}
template <typename T>
struct StepVjpArgs
{
   DevModel m;
   long B;
   T dt;
   const T *qd, *qdd;       // [B][nv] in the call's layout (v_bs, v_es)
   const T *gqn, *gqdn;     // cotangents of (dq', dqd'); either may be NULL (zero)
   T *gq, *gqd, *gqdd;      // any may be NULL
   const int *unowned;      // DoF indices no joint owns: zeros
   int n_unowned;
   long v_bs, v_es;
};
// One multi-DoF joint of one configuration (rows at `at`, element stride es).  di: the joint's entries of the DoF index map.
template <typename T, class IP>
MH_DEV void integrate_vjp_joint(int type, IP di, const StepVjpArgs<T> &A, long at, T dt, T hdd)
{
   const long es = A.v_es;
   const V3<T> z{T(0), T(0), T(0)};
   StepLin<T> L;
   step_lin_of_joint<T, IP>(type, di, A.qd + at, A.qdd + at, es, dt, hdd, L);
   const T *a = A.gqn ? A.gqn + at : nullptr, *b = A.gqdn ? A.gqdn + at : nullptr;
   const int k = dof_count(type);
   T ga[6], gb[6];
#pragma unroll
   for (int i = 0; i < 6; i++)
   {
      ga[i] = a && i < k ? a[di[i] * es] : T(0);
      gb[i] = b && i < k ? b[di[i] * es] : T(0);
   }
   V3<T> o0, o1, o2, o3, o4, o5;
   T oq[6], ov[6], oa[6];
   if (type == JT_SIXDOF)
   {
      step_apply_t<T>(L, dt, hdd, V3<T>{ga[0], ga[1], ga[2]}, V3<T>{ga[3], ga[4], ga[5]}, V3<T>{gb[0], gb[1], gb[2]}, V3<T>{gb[3], gb[4], gb[5]}, o0, o1,
                      o2, o3, o4, o5);
      oq[0] = o0.x, oq[1] = o0.y, oq[2] = o0.z, oq[3] = o1.x, oq[4] = o1.y, oq[5] = o1.z;
      ov[0] = o2.x, ov[1] = o2.y, ov[2] = o2.z, ov[3] = o3.x, ov[4] = o3.y, ov[5] = o3.z;
      oa[0] = o4.x, oa[1] = o4.y, oa[2] = o4.z, oa[3] = o5.x, oa[4] = o5.y, oa[5] = o5.z;
   }
   else if (type == JT_SPHERICAL)
   {
      step_apply_t<T>(L, dt, hdd, V3<T>{ga[0], ga[1], ga[2]}, z, V3<T>{gb[0], gb[1], gb[2]}, z, o0, o1, o2, o3, o4, o5);
      oq[0] = o0.x, oq[1] = o0.y, oq[2] = o0.z;
      ov[0] = o2.x, ov[1] = o2.y, ov[2] = o2.z;
      oa[0] = o4.x, oa[1] = o4.y, oa[2] = o4.z;
   }
   else
   { // planar (w_y, v_x, v_z): the restriction of the 6-DoF map to the XZ plane
      step_apply_t<T>(L, dt, hdd, V3<T>{T(0), ga[0], T(0)}, V3<T>{ga[1], T(0), ga[2]}, V3<T>{T(0), gb[0], T(0)}, V3<T>{gb[1], T(0), gb[2]}, o0, o1, o2, o3,
                      o4, o5);
      oq[0] = o0.y, oq[1] = o1.x, oq[2] = o1.z;
      ov[0] = o2.y, ov[1] = o3.x, ov[2] = o3.z;
      oa[0] = o4.y, oa[1] = o5.x, oa[2] = o5.z;
   }
#pragma unroll
   for (int i = 0; i < 6; i++)
      if (i < k)
      {
         const long e = at + di[i] * es;
         if (A.gq)
            A.gq[e] = oq[i];
         if (A.gqd)
            A.gqd[e] = ov[i];
         if (A.gqdd)
            A.gqdd[e] = oa[i];
      }
}
// a 1-DoF joint: entry e of every vector
template <typename T>
MH_DEV void integrate_vjp_one(const StepVjpArgs<T> &A, long e, T dt, T hdd)
{
   const T a = A.gqn ? A.gqn[e] : T(0), b = A.gqdn ? A.gqdn[e] : T(0);
   if (A.gq)
      A.gq[e] = a;
   if (A.gqd)
      A.gqd[e] = dt * a + b;
   if (A.gqdd)
      A.gqdd[e] = hdd * a + dt * b;
}
template <typename T>
MH_DEV void integrate_vjp_zero(const StepVjpArgs<T> &A, long at)
{
   for (int z = 0; z < A.n_unowned; z++)
   {
      const long e = at + A.unowned[z] * A.v_es;
      if (A.gq)
         A.gq[e] = T(0);
      if (A.gqd)
         A.gqd[e] = T(0);
      if (A.gqdd)
         A.gqdd[e] = T(0);
   }
}
// SoA: lane = configuration, joints looped, the joint's small matrices in registers.
template <typename T>
__global__ void __launch_bounds__(256) integrate_vjp_soa_kernel(StepVjpArgs<T> A)
{
   const DevModel &m = A.m;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map);
   const long nlanes = (long)gridDim.x * blockDim.x;
   const T dt = A.dt, hdd = T(0.5) * A.dt * A.dt;
   for (long cfg = (long)blockIdx.x * blockDim.x + threadIdx.x; cfg < A.B; cfg += nlanes)
   {
      const long at = cfg * A.v_bs;
      integrate_vjp_zero<T>(A, at);
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int type = mi[MI_TYPE];
         if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            integrate_vjp_one<T>(A, at + dof_map[mi[MI_DOF]] * A.v_es, dt, hdd);
         else if (type != JT_FIXED)
            integrate_vjp_joint<T, ciptr>(type, dof_map + mi[MI_DOF], A, at, dt, hdd);
      }
   }
}
// AoS: the thread mapping of integrate_aos_kernel.  A workgroup takes tiles of `tile` configurations; pass A: thread = (configuration,
// 1-DoF joint), the joint running fastest; pass B: thread = (configuration, multi-DoF joint).  The two joint lists are built once per
// workgroup in LDS; the unowned entries of a configuration are zeroed by one thread.
template <typename T>
__global__ void __launch_bounds__(256) integrate_vjp_aos_kernel(StepVjpArgs<T> A, int tile)
{
   extern __shared__ int lds_meta[]; // [n] v index of the 1-DoF joints ; [n] engine index of the others ; counts
   const DevModel &m = A.m;
   int *l1_v = lds_meta, *lm = lds_meta + m.n, *cnt = lds_meta + 2 * m.n;
   if (threadIdx.x == 0)
   {
      int n1 = 0, nm = 0;
      for (int j = 0; j < m.n; j++)
      {
         const int type = m.meta[j * MI_STRIDE + MI_TYPE];
         if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            l1_v[n1++] = m.dof_map[m.meta[j * MI_STRIDE + MI_DOF]];
         else if (type != JT_FIXED)
            lm[nm++] = j;
      }
      cnt[0] = n1, cnt[1] = nm;
   }
   __syncthreads();
   const unsigned n1 = (unsigned)cnt[0], nm = (unsigned)cnt[1];
   const T dt = A.dt, hdd = T(0.5) * A.dt * A.dt;
   const long ntiles = (A.B + tile - 1) / tile;
   for (long t = blockIdx.x; t < ntiles; t += gridDim.x)
   {
      const long cfg0 = t * tile;
      const unsigned rows = (unsigned)(A.B - cfg0 < (long)tile ? A.B - cfg0 : (long)tile);
      if (A.n_unowned > 0)
         for (unsigned u = threadIdx.x; u < rows; u += blockDim.x)
            integrate_vjp_zero<T>(A, (cfg0 + u) * A.v_bs);
      for (unsigned u = threadIdx.x; u < rows * n1; u += blockDim.x)
      {
         const unsigned lc = u / n1, k = u - lc * n1;
         integrate_vjp_one<T>(A, (cfg0 + lc) * A.v_bs + l1_v[k], dt, hdd);
      }
      for (unsigned u = threadIdx.x; u < rows * nm; u += blockDim.x)
      {
         const unsigned lc = u / nm, j = (unsigned)lm[u - lc * nm];
         const int *mi = m.meta + j * MI_STRIDE;
         integrate_vjp_joint<T, const int *>(mi[MI_TYPE], m.dof_map + mi[MI_DOF], A, (cfg0 + lc) * A.v_bs, dt, hdd);
      }
   }
}

// ---- Forward mode of the integrator: step_apply itself on directions (dq, dqd, dqdd) of one configuration, per joint, which gives the
// joint's entries of (dq', dqd') -- the blocks the assembly kernels above apply column by column, here applied once.  Its transpose is
// integrate_vjp_*.  A 1-DoF joint: dq' = dq + dt dqd + dt^2/2 dqdd, dqd' = dqd + dt dqdd.  At dt = 0 E and J_r are the identity and
// dq' = dq, dqd' = dqd come out exactly.
template <typename T>
struct StepJvpArgs
{
   DevModel m;
   long B;
   T dt;
   const T *qd, *qdd;       // [B][nv] in the call's layout (v_bs, v_es)
   const T *dq, *dqd, *dqdd; // directions; any may be NULL (zero, not read)
   T *dqn, *dqdn;           // (dq', dqd'); either may be NULL
   const int *unowned;      // DoF indices no joint owns: zeros
   int n_unowned;
   long v_bs, v_es;
};
// One multi-DoF joint of one configuration (rows at `at`, element stride es).  di: the joint's entries of the DoF index map.
template <typename T, class IP>
MH_DEV void integrate_jvp_joint(int type, IP di, const StepJvpArgs<T> &A, long at, T dt, T hdd)
{
   const long es = A.v_es;
   StepLin<T> L;
   step_lin_of_joint<T, IP>(type, di, A.qd + at, A.qdd + at, es, dt, hdd, L);
   const int k = dof_count(type);
   T x[6], eq[6], ev[6], oq[6], ov[6];
#pragma unroll
   for (int i = 0; i < 6; i++)
   {
      eq[i] = A.dq && i < k ? A.dq[at + di[i] * es] : T(0);
      ev[i] = A.dqd && i < k ? A.dqd[at + di[i] * es] : T(0);
      x[i] = A.dqdd && i < k ? A.dqdd[at + di[i] * es] : T(0);
   }
   step_column<T>(type, L, dt, hdd, x, eq, ev, oq, ov);
#pragma unroll
   for (int i = 0; i < 6; i++)
      if (i < k)
      {
         const long e = at + di[i] * es;
         if (A.dqn)
            A.dqn[e] = oq[i];
         if (A.dqdn)
            A.dqdn[e] = ov[i];
      }
}
// a 1-DoF joint: entry e of every vector
template <typename T>
MH_DEV void integrate_jvp_one(const StepJvpArgs<T> &A, long e, T dt, T hdd)
{
   const T a = A.dq ? A.dq[e] : T(0), b = A.dqd ? A.dqd[e] : T(0), c = A.dqdd ? A.dqdd[e] : T(0);
   if (A.dqn)
      A.dqn[e] = a + dt * b + hdd * c;
   if (A.dqdn)
      A.dqdn[e] = b + dt * c;
}
template <typename T>
MH_DEV void integrate_jvp_zero(const StepJvpArgs<T> &A, long at)
{
   for (int z = 0; z < A.n_unowned; z++)
   {
      const long e = at + A.unowned[z] * A.v_es;
      if (A.dqn)
         A.dqn[e] = T(0);
      if (A.dqdn)
         A.dqdn[e] = T(0);
   }
}
// SoA: lane = configuration, joints looped, the joint's small matrices in registers.
template <typename T>
__global__ void __launch_bounds__(256) integrate_jvp_soa_kernel(StepJvpArgs<T> A)
{
   const DevModel &m = A.m;
   const ciptr meta = as_const(m.meta), dof_map = as_const(m.dof_map);
   const long nlanes = (long)gridDim.x * blockDim.x;
   const T dt = A.dt, hdd = T(0.5) * A.dt * A.dt;
   for (long cfg = (long)blockIdx.x * blockDim.x + threadIdx.x; cfg < A.B; cfg += nlanes)
   {
      const long at = cfg * A.v_bs;
      integrate_jvp_zero<T>(A, at);
      for (int j = 0; j < m.n; j++)
      {
         ciptr mi = meta + j * MI_STRIDE;
         const int type = mi[MI_TYPE];
         if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            integrate_jvp_one<T>(A, at + dof_map[mi[MI_DOF]] * A.v_es, dt, hdd);
         else if (type != JT_FIXED)
            integrate_jvp_joint<T, ciptr>(type, dof_map + mi[MI_DOF], A, at, dt, hdd);
      }
   }
}
// AoS: the thread mapping of integrate_vjp_aos_kernel, joint lists in LDS.
template <typename T>
__global__ void __launch_bounds__(256) integrate_jvp_aos_kernel(StepJvpArgs<T> A, int tile)
{
   extern __shared__ int lds_meta[]; // [n] v index of the 1-DoF joints ; [n] engine index of the others ; counts
   const DevModel &m = A.m;
   int *l1_v = lds_meta, *lm = lds_meta + m.n, *cnt = lds_meta + 2 * m.n;
   if (threadIdx.x == 0)
   {
      int n1 = 0, nm = 0;
      for (int j = 0; j < m.n; j++)
      {
         const int type = m.meta[j * MI_STRIDE + MI_TYPE];
         if (type == JT_REVOLUTE || type == JT_PRISMATIC)
            l1_v[n1++] = m.dof_map[m.meta[j * MI_STRIDE + MI_DOF]];
         else if (type != JT_FIXED)
            lm[nm++] = j;
      }
      cnt[0] = n1, cnt[1] = nm;
   }
   __syncthreads();
   const unsigned n1 = (unsigned)cnt[0], nm = (unsigned)cnt[1];
   const T dt = A.dt, hdd = T(0.5) * A.dt * A.dt;
   const long ntiles = (A.B + tile - 1) / tile;
   for (long t = blockIdx.x; t < ntiles; t += gridDim.x)
   {
      const long cfg0 = t * tile;
      const unsigned rows = (unsigned)(A.B - cfg0 < (long)tile ? A.B - cfg0 : (long)tile);
      if (A.n_unowned > 0)
         for (unsigned u = threadIdx.x; u < rows; u += blockDim.x)
            integrate_jvp_zero<T>(A, (cfg0 + u) * A.v_bs);
      for (unsigned u = threadIdx.x; u < rows * n1; u += blockDim.x)
      {
         const unsigned lc = u / n1, k = u - lc * n1;
         integrate_jvp_one<T>(A, (cfg0 + lc) * A.v_bs + l1_v[k], dt, hdd);
      }
      for (unsigned u = threadIdx.x; u < rows * nm; u += blockDim.x)
      {
         const unsigned lc = u / nm, j = (unsigned)lm[u - lc * nm];
         const int *mi = m.meta + j * MI_STRIDE;
         integrate_jvp_joint<T, const int *>(mi[MI_TYPE], m.dof_map + mi[MI_DOF], A, (cfg0 + lc) * A.v_bs, dt, hdd);
      }
   }
}

// ------------------------------------------------------------------------------------------------ q (+) dq and q1 (-) q0
template <typename T>
struct ChartArgs
{
   DevModel m;
   long B;
   const T *a, *b; // add: q, dq; difference: q0, q1
   T *out;         // add: q_out; difference: dq_out
   const int *unowned;
   int n_unowned, soa;
   long q_bs, q_es, v_bs, v_es;
};
// item u of B * n -> (configuration, joint): the joint runs fastest in AoS, the configuration in SoA
template <typename T>
MH_DEV void chart_item(const ChartArgs<T> &A, long u, long n, long &cfg, int &j)
{
   if (A.soa)
      j = (int)(u / A.B), cfg = u - (long)j * A.B;
   else
      cfg = u / n, j = (int)(u - cfg * n);
}
template <typename T>
__global__ void __launch_bounds__(256) configuration_add_kernel(ChartArgs<T> A)
{
   const DevModel &m = A.m;
   const long total = A.B * m.n, nthreads = (long)gridDim.x * blockDim.x, qe = A.q_es, ve = A.v_es;
   for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += nthreads)
   {
      long cfg;
      int j;
      chart_item<T>(A, u, m.n, cfg, j);
      const int *mi = m.meta + j * MI_STRIDE;
      const int type = mi[MI_TYPE];
      const int *ci = m.cfg_map + mi[MI_CFG], *di = m.dof_map + mi[MI_DOF];
      const T *qr = A.a + cfg * A.q_bs, *dr = A.b + cfg * A.v_bs;
      T *qo = A.out + cfg * A.q_bs;
      if (type == JT_REVOLUTE || type == JT_PRISMATIC)
         qo[ci[0] * qe] = qr[ci[0] * qe] + dr[di[0] * ve];
      else if (type == JT_PLANAR)
      {
         const T pitch = qr[ci[0] * qe], px = qr[ci[1] * qe], pz = qr[ci[2] * qe];
         const T dx = dr[di[1] * ve], dz = dr[di[2] * ve];
         T s0, c0;
         sincos_t(pitch, s0, c0);
         qo[ci[0] * qe] = pitch + dr[di[0] * ve];
         qo[ci[1] * qe] = px + c0 * dx + s0 * dz;
         qo[ci[2] * qe] = pz - s0 * dx + c0 * dz;
      }
      else if (type == JT_SPHERICAL || type == JT_SIXDOF)
      { // integrate_sixdof with dt = 1 and no dt^2/2 term: Q' = Q exp(dth), p' = p + R(Q) dp
         T qx = qr[ci[0] * qe], qy = qr[ci[1] * qe], qz = qr[ci[2] * qe], qs = qr[ci[3] * qe];
         const bool six = type == JT_SIXDOF;
         V3<T> p{T(0), T(0), T(0)}, w{dr[di[0] * ve], dr[di[1] * ve], dr[di[2] * ve]}, v{T(0), T(0), T(0)};
         const V3<T> z{T(0), T(0), T(0)};
         if (six)
            p = V3<T>{qr[ci[4] * qe], qr[ci[5] * qe], qr[ci[6] * qe]}, v = V3<T>{dr[di[3] * ve], dr[di[4] * ve], dr[di[5] * ve]};
         integrate_sixdof<T>(T(1), T(0), qx, qy, qz, qs, p, w, v, z, z, nullptr);
         qo[ci[0] * qe] = qx, qo[ci[1] * qe] = qy, qo[ci[2] * qe] = qz, qo[ci[3] * qe] = qs;
         if (six)
            qo[ci[4] * qe] = p.x, qo[ci[5] * qe] = p.y, qo[ci[6] * qe] = p.z;
      }
   }
}
template <typename T>
__global__ void __launch_bounds__(256) configuration_difference_kernel(ChartArgs<T> A)
{
   const DevModel &m = A.m;
   const long total = A.B * m.n, nthreads = (long)gridDim.x * blockDim.x, qe = A.q_es, ve = A.v_es;
   const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
   for (long u = first; u < A.B * A.n_unowned; u += nthreads)
   {
      const long cfg = A.soa ? u % A.B : u / A.n_unowned;
      const int r = A.unowned[A.soa ? u / A.B : u % A.n_unowned];
      A.out[cfg * A.v_bs + r * ve] = T(0);
   }
   for (long u = first; u < total; u += nthreads)
   {
      long cfg;
      int j;
      chart_item<T>(A, u, m.n, cfg, j);
      const int *mi = m.meta + j * MI_STRIDE;
      const int type = mi[MI_TYPE];
      const int *ci = m.cfg_map + mi[MI_CFG], *di = m.dof_map + mi[MI_DOF];
      const T *q0 = A.a + cfg * A.q_bs, *q1 = A.b + cfg * A.q_bs;
      T *o = A.out + cfg * A.v_bs;
      if (type == JT_REVOLUTE || type == JT_PRISMATIC)
         o[di[0] * ve] = q1[ci[0] * qe] - q0[ci[0] * qe];
      else if (type == JT_PLANAR)
      {
         const T pitch = q0[ci[0] * qe];
         const T dx = q1[ci[1] * qe] - q0[ci[1] * qe], dz = q1[ci[2] * qe] - q0[ci[2] * qe];
         T s0, c0;
         sincos_t(pitch, s0, c0);
         o[di[0] * ve] = q1[ci[0] * qe] - pitch;
         o[di[1] * ve] = c0 * dx - s0 * dz;
         o[di[2] * ve] = s0 * dx + c0 * dz;
      }
      else if (type == JT_SPHERICAL || type == JT_SIXDOF)
      {
         T ax = q0[ci[0] * qe], ay = q0[ci[1] * qe], az = q0[ci[2] * qe], as = q0[ci[3] * qe];
         T bx = q1[ci[0] * qe], by = q1[ci[1] * qe], bz = q1[ci[2] * qe], bs = q1[ci[3] * qe];
         const T ia = T(1) / sqrt(ax * ax + ay * ay + az * az + as * as), ib = T(1) / sqrt(bx * bx + by * by + bz * bz + bs * bs);
         ax *= ia, ay *= ia, az *= ia, as *= ia, bx *= ib, by *= ib, bz *= ib, bs *= ib;
         // conj(Q0) Q1, then the rotation vector of the member of +-Q with s >= 0
         T x = as * bx - ax * bs - ay * bz + az * by;
         T y = as * by + ax * bz - ay * bs - az * bx;
         T z = as * bz - ax * by + ay * bx - az * bs;
         T s = as * bs + ax * bx + ay * by + az * bz;
         if (s < T(0))
            x = -x, y = -y, z = -z, s = -s;
         const T nn = sqrt(x * x + y * y + z * z);
         const T f = nn > T(0) ? T(2) * atan2(nn, s) / nn : T(2) / s;
         o[di[0] * ve] = f * x, o[di[1] * ve] = f * y, o[di[2] * ve] = f * z;
         if (type == JT_SIXDOF)
         {
            const M3<T> R0 = quat_to_R(ax, ay, az, as);
            const V3<T> dp = tmul(R0, V3<T>{q1[ci[4] * qe] - q0[ci[4] * qe], q1[ci[5] * qe] - q0[ci[5] * qe], q1[ci[6] * qe] - q0[ci[6] * qe]});
            o[di[3] * ve] = dp.x, o[di[4] * ve] = dp.y, o[di[5] * ve] = dp.z;
         }
      }
   }
}
} // namespace mh
