// pgo.hip -- joint refinement of a pose graph on SE(3)^N (the stage after chordal initialisation: so3.hip gives the
// rotations, pgo_trans.hip the positions for fixed rotations, this file minimises over both):
//     f(R, t) = 1/2 sum_e kappa_e | R_j - R_i Rt_e |_F^2  +  1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2,   e = (i -> j)
// as device callables for TNT (Objective, QuadraticModel, Retraction, block-Jacobi preconditioner; metric = coordinate dot).
// No gauge is fixed: the Hessian is semidefinite along the global motions, which STPCG copes with as it does in so3.hip.
//
// Point: 12N doubles [R | t], the first 9N in the layout of mi_so3n (row-major 3x3 blocks), the last 3N in the layout of
// mi_pgo_trans (N x 3 row-major).  Tangent: 6N doubles, node-major [xi_i (3), delta_i (3)]: R_i exp(hat xi_i), t_i + delta_i.
//
// With r_e = t_j - t_i - R_i tt_e, u_e = R_i' r_e, A_e = R_i hat(tt_e) (row r of A_e is row r of R_i crossed with tt_e):
//   gradient   g_xi_i    = vee(Q_i - Q_i') [rotation term, so3.hip]  +  sum_{e out of i} -tau_e tt_e x u_e
//              g_delta_i = sum_{e out of i} -tau_e r_e + sum_{e into i} tau_e r_e
//   Hessian    h_xi_i    = Hxx_i xi_i - K_i' delta_i - sum_slots kappa B_ij xi_j + sum_{out slots} (tau_e A_e)' delta_j
//              h_delta_i = degtau_i delta_i - K_i xi_i - sum_slots tau_e delta_nbr + sum_{in slots} (tau_e A_e) xi_k
//     Hxx_i = D_i [so3.hip] + sum_{e out of i} tau_e [ |tt|^2 I - tt tt' + (u.tt) I - 1/2 (u tt' + tt u') ]
//     K_i   = R_i hat(sum_{e out of i} tau_e tt_e),  degtau_i = sum over the slots of i of tau_e
// (the second-order part comes from exp(hat xi) tt = tt + xi x tt + 1/2 xi x (xi x tt): the Hessian of f along the retraction,
// tests/test_cpu_pgo_fd.py).  f is 1/4 of the sum over INCIDENCES of kappa |R_i - R_j S|^2 + tau |r_e|^2 (every edge is seen
// from both ends), as in so3.hip.
//
// Layout (pgo_pack.h): the SELL-64-sigma incidence layout of so3_pack.h with per-slot streams rinc (9), tinc (3), kinc, tauinc
// and the slot words.  What the model pass writes, all component-major per slice entry and streamed non-temporally:
//   Bblk (9 per slot)  kappa B_ij                       Gblk (9 per slot)  (tau A_e)' at an out slot, tau A_e at an in slot
//   Nsl (19 per node, slice order)  Hxx_i (9), K_i (9), degtau_i
//   Minv (18 per node, node order)  Hxx_i^-1, I / degtau_i: the 2N inverse blocks of mi_precon_create_block3 on the 6N tangent.
//     A block that cannot be inverted (determinant 0 or not finite: a node without weight) is replaced by the identity.
// k_pgo_model<FORM>: one lane per node in slice order, the walk of k_so3_model; FORM = objective only / gradient only / model /
//   gradient and inverse blocks (the trial chain's |M^-1 grad| at the trial point).  Contraction is off in the whole pass: the
//   forms leave the same bits.  No atomics; the objective's partial rows go to ctx->partials2 in the layout of k_so3_model.
//   Algorithmic bytes of the model form: 116 per slot read (72 rinc + 24 tinc + 16 weights + 4 nbr) + 144 per slot written
//   + 96 gathered per live slot (R_j, t_j) + N (4 + 96 read + 48 + 152 + 144 written).
// k_pgo_hvp<DOTS>: h = H eta in one pass over the slots, one lane per node, the walk and the partial rows of k_bsr3_spmv.
//   Algorithmic bytes: 160 per slot (72 Bblk + 72 Gblk + 8 tau + 4 nbr + 4 word) + 48 gathered per slot (eta_nbr)
//   + N (4 + 152 + 48 read + 48 written).
// k_pgo_retract: Rodrigues on R with the series switch of k_so3_retract, t + delta.
#include <algorithm>
#include <cmath>

#include "mi_internal.h"
#include "pgo_pack.h"

using namespace mi;

namespace {

struct PgoView {
  size_t N, nslices;
  const long long *__restrict__ slice_ptr;
  const int *__restrict__ perm;       // node owned by (slice, lane), -1: padding lane
  const int *__restrict__ nbr;        // neighbour node (padding: own node)
  const uint32_t *__restrict__ slot;  // edge << 1 | (the slot's node is the first node of the edge)
  const double *__restrict__ rinc;    // 9 per slot
  const double *__restrict__ tinc;    // 3 per slot
  const double *__restrict__ kinc;
  const double *__restrict__ tauinc;
};
struct PgoModelOut {
  double *__restrict__ grad;  // 6N
  double *__restrict__ Bblk;  // padded * 9
  double *__restrict__ Gblk;  // padded * 9
  double *__restrict__ Nsl;   // nslices * 19 * 64
  double *__restrict__ Minv;  // 18N
};
constexpr int kNodeComps = 19;

// (the small 3x3 helpers of so3.hip, restated)
__device__ __forceinline__ void mat3_mul(const double *A, const double *B, double *C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void mat3_mul_at(const double *A, const double *B, double *C) {  // A' B
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void vee_skew2(const double *T, double *o) {
  o[0] = T[7] - T[5];
  o[1] = T[2] - T[6];
  o[2] = T[3] - T[1];
}
// M = Q hat(e_m)
__device__ __forceinline__ void q_hat_basis(const double *Q, int m, double *M) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double q0 = Q[r * 3], q1 = Q[r * 3 + 1], q2 = Q[r * 3 + 2];
    if (m == 0) { M[r * 3] = 0; M[r * 3 + 1] = q2; M[r * 3 + 2] = -q1; }
    else if (m == 1) { M[r * 3] = -q2; M[r * 3 + 1] = 0; M[r * 3 + 2] = q0; }
    else { M[r * 3] = q1; M[r * 3 + 1] = -q0; M[r * 3 + 2] = 0; }
  }
}
// A = M hat(x): row r of M crossed with x
__device__ __forceinline__ void mat_hat(const double *M, double x0, double x1, double x2, double *A) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = M[r * 3], b = M[r * 3 + 1], c = M[r * 3 + 2];
    A[r * 3] = b * x2 - c * x1;
    A[r * 3 + 1] = c * x0 - a * x2;
    A[r * 3 + 2] = a * x1 - b * x0;
  }
}
// the inverse of a symmetric 3x3 block given by its upper triangle, or the identity where it has none
__device__ __forceinline__ void sym3_inverse_or_identity(double a, double b, double c, double e, double f, double g, double *o) {
#pragma clang fp contract(off)
  const double c00 = e * g - f * f, c01 = c * f - b * g, c02 = b * f - c * e;
  const double c11 = a * g - c * c, c12 = b * c - a * f, c22 = a * e - b * b;
  const double det = a * c00 + b * c01 + c * c02;
  if (det == 0.0 || !(fabs(det) <= 1.79769313486231571e308)) {
    o[0] = 1; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 1; o[5] = 0; o[6] = 0; o[7] = 0; o[8] = 1;
    return;
  }
  o[0] = c00 / det; o[1] = c01 / det; o[2] = c02 / det;
  o[3] = c01 / det; o[4] = c11 / det; o[5] = c12 / det;
  o[6] = c02 / det; o[7] = c12 / det; o[8] = c22 / det;
}

enum { PGO_OBJECTIVE = 0, PGO_MODEL = 1, PGO_GRAD = 2, PGO_GRAD_PRECON = 3 };

template <int FORM>
__device__ __forceinline__ void pgo_model_slice(const PgoView &v, const double *__restrict__ x, const PgoModelOut &o, size_t slice,
                                                int lane, double &facc) {
#pragma clang fp contract(off)
  constexpr bool kBlocks = FORM == PGO_MODEL;                             // the slot and node blocks of the Hessian
  constexpr bool kCurv = FORM == PGO_MODEL || FORM == PGO_GRAD_PRECON;   // the diagonal blocks and their inverses
  if (slice >= v.nslices) return;
  const int node = v.perm[slice * 64 + lane];
  const bool live = node >= 0;
  const size_t i = live ? (size_t)node : 0;
  const double *__restrict__ R = x, *__restrict__ t = x + 9 * v.N;
  double Ri[9], ti[3];
#pragma unroll
  for (int c = 0; c < 9; ++c) Ri[c] = live ? R[9 * i + c] : (c % 4 == 0 ? 1.0 : 0.0);
#pragma unroll
  for (int c = 0; c < 3; ++c) ti[c] = live ? t[3 * i + c] : 0.0;
  double EG[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double gx[3] = {0, 0, 0}, gd[3] = {0, 0, 0};
  double degk = 0, degt = 0;
  double T[6] = {0, 0, 0, 0, 0, 0};  // the translation term's part of Hxx: entries 00, 01, 02, 11, 12, 22
  double stt[3] = {0, 0, 0};         // sum over the out slots of tau tt
  const long long b0 = v.slice_ptr[slice], b1 = v.slice_ptr[slice + 1];
  for (long long k = b0; k < b1; ++k) {
    const size_t e0 = (size_t)k * 64 + lane;
    const double ke = __builtin_nontemporal_load(v.kinc + e0), te = __builtin_nontemporal_load(v.tauinc + e0);
    double Bk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Gk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live && (ke != 0 || te != 0)) {
      const size_t j = (size_t)__builtin_nontemporal_load(v.nbr + e0);
      const bool first = (__builtin_nontemporal_load(v.slot + e0) & 1u) != 0;
      double Rj[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) Rj[c] = R[9 * j + c];
      if (ke != 0) {
        double S[9], RjS[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) S[c] = __builtin_nontemporal_load(v.rinc + ((size_t)k * 9 + c) * 64 + lane);
        mat3_mul(Rj, S, RjS);
        double q = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          const double d = Ri[c] - RjS[c];
          EG[c] += ke * d;
          q += d * d;
        }
        facc += ke * q;
        degk += ke;
        if (kBlocks) {
          double Q[9];
          mat3_mul_at(Ri, Rj, Q);
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            double M[9], MS[9], col[3];
            q_hat_basis(Q, m, M);
            mat3_mul(M, S, MS);
            vee_skew2(MS, col);
            Bk[0 * 3 + m] = ke * col[0];
            Bk[1 * 3 + m] = ke * col[1];
            Bk[2 * 3 + m] = ke * col[2];
          }
        }
      }
      if (te != 0) {
        const double *Tp = v.tinc + (size_t)k * 3 * 64 + lane;
        const double a0 = __builtin_nontemporal_load(Tp), a1 = __builtin_nontemporal_load(Tp + 64),
                     a2 = __builtin_nontemporal_load(Tp + 128);
        const double tj0 = t[3 * j], tj1 = t[3 * j + 1], tj2 = t[3 * j + 2];
        // r_e with the first node's rotation: the lane's own at an out slot, the neighbour's at an in slot
        const double *Rf = first ? Ri : Rj;
        const double v0 = Rf[0] * a0 + Rf[1] * a1 + Rf[2] * a2, v1 = Rf[3] * a0 + Rf[4] * a1 + Rf[5] * a2,
                     v2 = Rf[6] * a0 + Rf[7] * a1 + Rf[8] * a2;
        const double sgn = first ? 1.0 : -1.0;  // t_j - t_i at an out slot, t_i - t_j at an in slot
        const double r0 = sgn * (tj0 - ti[0]) - v0, r1 = sgn * (tj1 - ti[1]) - v1, r2 = sgn * (tj2 - ti[2]) - v2;
        facc += te * ((r0 * r0 + r1 * r1) + r2 * r2);
        degt += te;
        gd[0] -= sgn * (te * r0); gd[1] -= sgn * (te * r1); gd[2] -= sgn * (te * r2);
        double A[9];
        if (first || kBlocks) mat_hat(Rf, a0, a1, a2, A);
        if (first) {
          const double u0 = Ri[0] * r0 + Ri[3] * r1 + Ri[6] * r2, u1 = Ri[1] * r0 + Ri[4] * r1 + Ri[7] * r2,
                       u2 = Ri[2] * r0 + Ri[5] * r1 + Ri[8] * r2;
          gx[0] -= te * (a1 * u2 - a2 * u1);
          gx[1] -= te * (a2 * u0 - a0 * u2);
          gx[2] -= te * (a0 * u1 - a1 * u0);
          if (kCurv) {
            const double aa = (a0 * a0 + a1 * a1) + a2 * a2, ua = (u0 * a0 + u1 * a1) + u2 * a2, d = aa + ua;
            T[0] += te * (d - a0 * a0 - u0 * a0);
            T[1] += te * (-a0 * a1 - .5 * (u0 * a1 + a0 * u1));
            T[2] += te * (-a0 * a2 - .5 * (u0 * a2 + a0 * u2));
            T[3] += te * (d - a1 * a1 - u1 * a1);
            T[4] += te * (-a1 * a2 - .5 * (u1 * a2 + a1 * u2));
            T[5] += te * (d - a2 * a2 - u2 * a2);
            stt[0] += te * a0; stt[1] += te * a1; stt[2] += te * a2;
          }
        }
        if (kBlocks) {
          if (first) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int c = 0; c < 3; ++c) Gk[r * 3 + c] = te * A[c * 3 + r];
          } else {
#pragma unroll
            for (int c = 0; c < 9; ++c) Gk[c] = te * A[c];
          }
        }
      }
    }
    if (kBlocks) {
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        __builtin_nontemporal_store(Bk[c], o.Bblk + ((size_t)k * 9 + c) * 64 + lane);
        __builtin_nontemporal_store(Gk[c], o.Gblk + ((size_t)k * 9 + c) * 64 + lane);
      }
    }
  }
  if (FORM == PGO_OBJECTIVE) return;
  if (!live) {
    if (kBlocks) {
#pragma unroll
      for (int c = 0; c < kNodeComps; ++c) __builtin_nontemporal_store(0.0, o.Nsl + (slice * kNodeComps + c) * 64 + lane);
    }
    return;
  }
  double Q[9], gr[3];
  mat3_mul_at(Ri, EG, Q);
  vee_skew2(Q, gr);
  double *g = o.grad + 6 * i;
  g[0] = gr[0] + gx[0]; g[1] = gr[1] + gx[1]; g[2] = gr[2] + gx[2];
  g[3] = gd[0]; g[4] = gd[1]; g[5] = gd[2];
  if (!kCurv) return;
  double C[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) C[a * 3 + b] = .5 * (Q[a * 3 + b] + Q[b * 3 + a]);
  const double tr = C[0] + C[4] + C[8], d = 2 * degk - tr;
  const double a = (d + C[0]) + T[0], b = C[1] + T[1], c = C[2] + T[2], e = (d + C[4]) + T[3], f = C[5] + T[4],
               gg = (d + C[8]) + T[5];
  if (kBlocks) {
    double K[9];
    mat_hat(Ri, stt[0], stt[1], stt[2], K);
    const double dd[9] = {a, b, c, b, e, f, c, f, gg};
    double *Np = o.Nsl + slice * kNodeComps * 64 + lane;
#pragma unroll
    for (int q = 0; q < 9; ++q) __builtin_nontemporal_store(dd[q], Np + q * 64);
#pragma unroll
    for (int q = 0; q < 9; ++q) __builtin_nontemporal_store(K[q], Np + (9 + q) * 64);
    __builtin_nontemporal_store(degt, Np + 18 * 64);
  }
  double *Mi = o.Minv + 18 * i;
  double inv[9];
  sym3_inverse_or_identity(a, b, c, e, f, gg, inv);
#pragma unroll
  for (int q = 0; q < 9; ++q) Mi[q] = inv[q];
  const double id = degt > 0 ? 1.0 / degt : 1.0;
  Mi[9] = id; Mi[10] = 0; Mi[11] = 0; Mi[12] = 0; Mi[13] = id; Mi[14] = 0; Mi[15] = 0; Mi[16] = 0; Mi[17] = id;
}

// one workgroup = 4 slices; workgroup b leaves its objective partial in row b % kMaxRows of component b / kMaxRows
// (k_so3_model's layout: pgo_rows_to_slot)
template <int FORM>
__global__ __launch_bounds__(256) void k_pgo_model(PgoView v, const double *__restrict__ x, PgoModelOut o,
                                                   double *__restrict__ fpartials) {
  __shared__ double flds[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double facc = 0;
  const size_t ngroups = (v.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) pgo_model_slice<FORM>(v, x, o, grp * 4 + w, lane, facc);
  facc = wave_reduce_sum(facc);
  if (lane == 0) flds[w] = facc;
  __syncthreads();
  if (threadIdx.x == 0) {
    fpartials[(size_t)(blockIdx.x / kMaxRows) * kMaxRows + blockIdx.x % kMaxRows] = (flds[0] + flds[1]) + (flds[2] + flds[3]);
    // the rows of the last component past the last workgroup read as zero
    const size_t total = (size_t)((gridDim.x + kMaxRows - 1) / kMaxRows) * kMaxRows, z = (size_t)gridDim.x + blockIdx.x;
    if (z < total) fpartials[z] = 0.0;
  }
}
// dst[0] = src[0] + ... + src[k-1] in index order (one thread)
__global__ void k_pgo_sum_slots(const double *__restrict__ src, int k, double *__restrict__ dst) {
  double s = 0;
  for (int i = 0; i < k; ++i) s += src[i];
  dst[0] = s;
}

// h = H eta, fused with the three curvature dots (one 1024-thread workgroup = 16 slices, the walk of k_bsr3_spmv)
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void k_pgo_hvp(PgoView v, const CgState *__restrict__ st, const double *__restrict__ Nsl,
                                                    const double *__restrict__ Bblk, const double *__restrict__ Gblk,
                                                    const double *__restrict__ eta, double *__restrict__ h,
                                                    double *__restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double lds[3 * kWaves];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double a[3] = {0, 0, 0};
  const size_t ngroups = (v.nslices + kWaves - 1) / kWaves;
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t g0 = (ngroups * lb) / nb, g1 = (ngroups * (lb + 1)) / nb;
  for (size_t g = g0; g < g1; ++g) {
    const size_t slice = g * kWaves + w;
    if (slice >= v.nslices) continue;
    const int node = v.perm[slice * 64 + lane];
    if (node < 0) continue;
    const size_t i = (size_t)node;
    double x[6];
    {
      const double2 p0 = *reinterpret_cast<const double2 *>(eta + 6 * i), p1 = *reinterpret_cast<const double2 *>(eta + 6 * i + 2),
                    p2 = *reinterpret_cast<const double2 *>(eta + 6 * i + 4);
      x[0] = p0.x; x[1] = p0.y; x[2] = p1.x; x[3] = p1.y; x[4] = p2.x; x[5] = p2.y;
    }
    const double *D = Nsl + slice * kNodeComps * 64 + lane;
    double hv[6];
    {
      double H[9], K[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) H[c] = __builtin_nontemporal_load(D + c * 64);
#pragma unroll
      for (int c = 0; c < 9; ++c) K[c] = __builtin_nontemporal_load(D + (9 + c) * 64);
      const double dt = __builtin_nontemporal_load(D + 18 * 64);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        hv[r] = (H[r * 3] * x[0] + H[r * 3 + 1] * x[1] + H[r * 3 + 2] * x[2]) - (K[r] * x[3] + K[3 + r] * x[4] + K[6 + r] * x[5]);
        hv[3 + r] = dt * x[3 + r] - (K[r * 3] * x[0] + K[r * 3 + 1] * x[1] + K[r * 3 + 2] * x[2]);
      }
    }
    const long long b0 = v.slice_ptr[slice], b1 = v.slice_ptr[slice + 1];
    for (long long k = b0; k < b1; ++k) {
      const size_t e0 = (size_t)k * 64 + lane;
      const size_t j = (size_t)__builtin_nontemporal_load(v.nbr + e0);
      const bool first = (__builtin_nontemporal_load(v.slot + e0) & 1u) != 0;
      const double te = __builtin_nontemporal_load(v.tauinc + e0);
      const double2 q0 = *reinterpret_cast<const double2 *>(eta + 6 * j), q1 = *reinterpret_cast<const double2 *>(eta + 6 * j + 2),
                    q2 = *reinterpret_cast<const double2 *>(eta + 6 * j + 4);
      const double y0 = q0.x, y1 = q0.y, y2 = q1.x, y3 = q1.y, y4 = q2.x, y5 = q2.y;
      const double *B = Bblk + (size_t)k * 9 * 64 + lane, *G = Gblk + (size_t)k * 9 * 64 + lane;
      // (tau A)' delta_j into the xi rows at an out slot, (tau A) xi_k into the delta rows at an in slot
      const double z0 = first ? y3 : y0, z1 = first ? y4 : y1, z2 = first ? y5 : y2;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double bx = __builtin_nontemporal_load(B + (r * 3) * 64) * y0 + __builtin_nontemporal_load(B + (r * 3 + 1) * 64) * y1 +
                          __builtin_nontemporal_load(B + (r * 3 + 2) * 64) * y2;
        const double gz = __builtin_nontemporal_load(G + (r * 3) * 64) * z0 + __builtin_nontemporal_load(G + (r * 3 + 1) * 64) * z1 +
                          __builtin_nontemporal_load(G + (r * 3 + 2) * 64) * z2;
        hv[r] -= bx;
        hv[r] += first ? gz : 0.0;
        hv[3 + r] += first ? 0.0 : gz;
      }
      hv[3] -= te * y3; hv[4] -= te * y4; hv[5] -= te * y5;
    }
    *reinterpret_cast<double2 *>(h + 6 * i) = make_double2(hv[0], hv[1]);
    *reinterpret_cast<double2 *>(h + 6 * i + 2) = make_double2(hv[2], hv[3]);
    *reinterpret_cast<double2 *>(h + 6 * i + 4) = make_double2(hv[4], hv[5]);
    if (DOTS) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        a[0] += x[c] * hv[c];
        a[1] += hv[c] * hv[c];
        a[2] += x[c] * x[c];
      }
    }
  }
  if (DOTS) block_partials_store<3>(a, lds, partials);
}

// y = [R_i exp(hat xi_i) | t_i + delta_i]  (Rodrigues; the series switch of k_so3_retract)
// (80 scalar registers, as k_so3_retract: two 1024-thread workgroups per CU need all 8 wave slots per SIMD)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(80))) void k_pgo_retract(size_t N, const double *__restrict__ x, const double *__restrict__ eta,
                                                        double *__restrict__ y) {
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
    const double x0 = eta[6 * i], x1 = eta[6 * i + 1], x2 = eta[6 * i + 2];
    const double th2 = x0 * x0 + x1 * x1 + x2 * x2, th = sqrt(th2);
    double a, b;
    if (th < 1e-4) {
      a = 1 - th2 / 6 + th2 * th2 / 120;
      b = .5 - th2 / 24 + th2 * th2 / 720;
    } else {
      a = sin(th) / th;
      b = (1 - cos(th)) / th2;
    }
    const double K[9] = {0, -x2, x1, x2, 0, -x0, -x1, x0, 0};
    double K2[9], Ex[9], Ri[9], Yi[9];
    mat3_mul(K, K, K2);
#pragma unroll
    for (int c = 0; c < 9; ++c) Ex[c] = a * K[c] + b * K2[c];
    Ex[0] += 1; Ex[4] += 1; Ex[8] += 1;
#pragma unroll
    for (int c = 0; c < 9; ++c) Ri[c] = x[9 * i + c];
    mat3_mul(Ri, Ex, Yi);
#pragma unroll
    for (int c = 0; c < 9; ++c) y[9 * i + c] = Yi[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) y[9 * N + 3 * i + c] = x[9 * N + 3 * i + c] + eta[6 * i + 3 + c];
  }
}

}  // namespace

struct mi_pgo {
  mi_ctx *ctx = nullptr;
  size_t N = 0, E = 0, nslices = 0, nnzb = 0, padded = 0;
  DevPtr<long long> slice_ptr;
  DevPtr<int> perm, nbr;
  DevPtr<uint32_t> slot;
  DevPtr<double> rinc, tinc, kinc, tauinc;
  DevPtr<double> Bblk, Gblk, Nsl;           // padded * 9 each; nslices * 19 * 64
  Owned<mi_vec> Minv;                       // 18N: the inverse blocks at the point of the model
  Owned<mi_vec> Minv_trial, grad_trial;     // 18N, 6N: what the trial chain leaves at the trial point
  Owned<mi_vec> Hh, Pg;                     // 6N each: Hess h and M^-1 grad of the trial chain
  mi_op hess;                               // lent out as `borrowed`
  Owned<mi_precon> bj;                      // mi_precon_create_block3(ctx, Minv): lent out as `borrowed`
  Owned<mi_precon> bj_trial;                // the same over Minv_trial: the trial chain's M^-1 at the trial point
  const mi_vec *x = nullptr;                // the point the model is bound to, by handle AND serial (mi::bound_to)
  uint64_t x_serial = 0;
};

namespace {

// Without a device the answer is MI_ERR_NO_DEVICE whatever the arguments (no context can exist); with one, a null
// argument is the usual MI_ERR_INVALID_ARGUMENT.
#define PGO_REQUIRE_ARGS(COND)                 \
  do {                                         \
    if (!(COND)) {                             \
      MI_TRY(ensure_device());                 \
      MI_REQUIRE(false, "null argument");      \
    }                                          \
  } while (0)

// workgroups of the assembly: one per group of 4 slices while their objective partials fit 8 components of kMaxRows rows,
// a grid-stride walk beyond (k_so3_model's rule)
constexpr int kPgoModelComps = 8;
int model_grid(const mi_pgo *p) {
  return (int)std::max<size_t>(1, std::min<size_t>((p->nslices + 3) / 4, (size_t)kPgoModelComps * kMaxRows));
}
PgoView view(const mi_pgo *p) {
  return PgoView{p->N, p->nslices, p->slice_ptr.get(), p->perm.get(), p->nbr.get(), p->slot.get(),
                 p->rinc.get(), p->tinc.get(), p->kinc.get(), p->tauinc.get()};
}
int check_point(const mi_pgo *p, const mi_vec *x, const char *what) {
  MI_REQUIRE(x->ctx == p->ctx && x->n == 12 * p->N, "%s must hold 12N doubles [R | t]", what);
  return MI_OK;
}
int check_tangent(const mi_pgo *p, const mi_vec *v, const char *what) {
  MI_REQUIRE(v->ctx == p->ctx && v->n == 6 * p->N, "%s must hold 6N doubles", what);
  return MI_OK;
}
// the assembly at x in one of its forms; the objective's partial rows into ctx->partials2
int launch_assembly(mi_pgo *p, int form, const double *x, double *grad, double *Minv) {
  mi_ctx *ctx = p->ctx;
  const int grid = model_grid(p);
  const PgoModelOut o{grad, p->Bblk.get(), p->Gblk.get(), p->Nsl.get(), Minv};
  KScope ks(ctx, form == PGO_MODEL ? MI_K_PGO_MODEL : MI_K_PGO_GRAD);
  switch (form) {
    case PGO_OBJECTIVE:
      hipLaunchKernelGGL(k_pgo_model<PGO_OBJECTIVE>, dim3(grid), dim3(256), 0, ctx->stream, view(p), x, o, ctx->partials2);
      break;
    case PGO_MODEL:
      hipLaunchKernelGGL(k_pgo_model<PGO_MODEL>, dim3(grid), dim3(256), 0, ctx->stream, view(p), x, o, ctx->partials2);
      break;
    case PGO_GRAD:
      hipLaunchKernelGGL(k_pgo_model<PGO_GRAD>, dim3(grid), dim3(256), 0, ctx->stream, view(p), x, o, ctx->partials2);
      break;
    default:
      hipLaunchKernelGGL(k_pgo_model<PGO_GRAD_PRECON>, dim3(grid), dim3(256), 0, ctx->stream, view(p), x, o, ctx->partials2);
      break;
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}
// the objective partial rows of the last assembly -> one sum in *slot (4 f), in the order mi_pgo_objective uses
int rows_to_slot(mi_pgo *p, double *slot) {
  mi_ctx *ctx = p->ctx;
  const int grid = model_grid(p), comps = (grid + kMaxRows - 1) / kMaxRows;
  if (comps == 1) return reduce_rows_allreduce(ctx, ctx->partials2, grid, 1, slot);
  double *tmp = ctx->scalars + SLOT_RAW;  // (free outside mi_stiefel_gram)
  MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, kMaxRows, comps, tmp));
  hipLaunchKernelGGL(k_pgo_sum_slots, dim3(1), dim3(1), 0, ctx->stream, (const double *)tmp, comps, slot);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
// gated: the fused pass does nothing once the solve on this context has left CG_RUN (mi_op::apply_dots)
int pgo_apply_common(mi_op *self, const mi_vec *in, mi_vec *out, bool dots, int *nparts, bool gated = true) {
  mi_pgo *p = (mi_pgo *)self->impl;
  mi_ctx *ctx = p->ctx;
  MI_REQUIRE(((uintptr_t)in->d | (uintptr_t)out->d) % 16 == 0, "the joint Hessian reads and writes 16-byte aligned tangents");
  const int grid = uniform_grid(ctx, (p->nslices + kWaves - 1) / kWaves);
  KScope ks(ctx, MI_K_PGO_HVP);
  if (dots)
    hipLaunchKernelGGL(k_pgo_hvp<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, view(p),
                       gated ? ctx->cg_live : (const CgState *)nullptr, (const double *)p->Nsl.get(), (const double *)p->Bblk.get(), (const double *)p->Gblk.get(),
                       (const double *)in->d, out->d, ctx->partials);
  else
    hipLaunchKernelGGL(k_pgo_hvp<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, view(p), (const CgState *)nullptr,
                       (const double *)p->Nsl.get(), (const double *)p->Bblk.get(), (const double *)p->Gblk.get(),
                       (const double *)in->d, out->d, (double *)nullptr);
  if (nparts) *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}
int pgo_apply(mi_op *self, const mi_vec *in, mi_vec *out) { return pgo_apply_common(self, in, out, false, nullptr); }
int pgo_apply_dots(mi_op *self, const mi_vec *in, mi_vec *out, int *np) { return pgo_apply_common(self, in, out, true, np); }
int launch_retract(mi_pgo *p, const mi_vec *x, const mi_vec *eta, mi_vec *y) {
  touch(y);
  KScope ks(p->ctx, MI_K_PGO_RETRACT);
  hipLaunchKernelGGL(k_pgo_retract, dim3(grid_for(p->ctx, p->N, 1)), dim3(kBlock), 0, p->ctx->stream, p->N, (const double *)x->d,
                     (const double *)eta->d, y->d);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
// the trial arrays, made by the first mi_pgo_trial (a client of mi_pgo_model alone allocates none of them)
int ensure_trial_arrays(mi_pgo *p) {
  if (p->grad_trial) return MI_OK;
  Owned<mi_vec> Minv, grad, Hh, Pg;
  MI_TRY(vec_alloc(p->ctx, 18 * p->N, Minv));
  MI_TRY(vec_alloc(p->ctx, 6 * p->N, grad));
  MI_TRY(vec_alloc(p->ctx, 6 * p->N, Hh));
  MI_TRY(vec_alloc(p->ctx, 6 * p->N, Pg));
  mi_precon *bj = nullptr;
  MI_TRY(mi_precon_create_block3(p->ctx, Minv.get(), &bj));
  p->bj_trial.reset(bj);
  p->Minv_trial = std::move(Minv), p->grad_trial = std::move(grad), p->Hh = std::move(Hh), p->Pg = std::move(Pg);
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_pgo_create(mi_ctx *ctx, size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *tt,
                  const double *kappa, const double *tau, mi_pgo **out) {
  PGO_REQUIRE_ARGS(ctx && out && (E == 0 || (ei && ej && Rt && tt && kappa && tau)));
  MI_REQUIRE(!ctx->uniform_grid && !ctx->comm, "the joint pose-graph problem is single-context");
  PgoPack P;
  std::string err;
  MI_REQUIRE(pgo_pack(N, E, ei, ej, Rt, tt, kappa, tau, P, err) == 0, "%s", err.c_str());
  auto p = std::make_unique<mi_pgo>();  // (everything below is owned: an early return releases what was made)
  p->ctx = ctx;
  p->N = N, p->E = E, p->nslices = P.nslices, p->nnzb = P.nnzb, p->padded = P.padded;
  MI_TRY(dev_upload(p->slice_ptr, P.slice_ptr.data(), P.slice_ptr.size()));
  MI_TRY(dev_upload(p->perm, P.perm.data(), P.perm.size()));
  MI_TRY(dev_upload(p->nbr, P.nbr.data(), P.padded));
  MI_TRY(dev_upload(p->slot, P.slot.data(), P.slot.size()));
  MI_TRY(dev_upload(p->rinc, P.rinc.data(), P.rinc.size()));
  MI_TRY(dev_upload(p->tinc, P.tinc.data(), P.tinc.size()));
  MI_TRY(dev_upload(p->kinc, P.kinc.data(), P.kinc.size()));
  MI_TRY(dev_upload(p->tauinc, P.tauinc.data(), P.tauinc.size()));
  MI_TRY(dev_alloc(p->Bblk, P.padded * 9));
  MI_TRY(dev_alloc(p->Gblk, P.padded * 9));
  MI_TRY(dev_alloc(p->Nsl, P.nslices * kNodeComps * 64));
  MI_TRY(vec_alloc(ctx, 18 * N, p->Minv));
  p->hess.ctx = ctx, p->hess.n = 6 * N, p->hess.n_out = 0, p->hess.impl = p.get(), p->hess.borrowed = true;
  p->hess.apply = pgo_apply, p->hess.apply_dots = pgo_apply_dots;
  mi_precon *bj = nullptr;
  MI_TRY(mi_precon_create_block3(ctx, p->Minv.get(), &bj));  // fusable 3x3 block-Jacobi: 2N blocks on the 6N tangent
  p->bj.reset(bj);
  bj->borrowed = true;
  *out = p.release();
  return MI_OK;
}

int mi_pgo_destroy(mi_pgo *p) {
  if (!p) return MI_OK;
  (void)hipStreamSynchronize(p->ctx->stream);
  delete p;
  return MI_OK;
}

int mi_pgo_objective(mi_pgo *p, const mi_vec *x, double *f) {
  PGO_REQUIRE_ARGS(p && x && f);
  MI_TRY(check_point(p, x, "x"));
  mi_ctx *ctx = p->ctx;
  MI_TRY(launch_assembly(p, PGO_OBJECTIVE, x->d, nullptr, nullptr));
  MI_TRY(rows_to_slot(p, ctx->scalars + SLOT_MISC));
  double s = 0;
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, 1, &s));
  *f = .25 * s;  // (every edge from both ends)
  return MI_OK;
}

int mi_pgo_gradient(mi_pgo *p, const mi_vec *x, mi_vec *grad) {
  PGO_REQUIRE_ARGS(p && x && grad);
  MI_TRY(check_point(p, x, "x"));
  MI_TRY(check_tangent(p, grad, "the gradient"));
  touch(grad);
  return launch_assembly(p, PGO_GRAD, x->d, grad->d, nullptr);
}

int mi_pgo_model(mi_pgo *p, const mi_vec *x, mi_vec *grad, mi_op **hess, mi_precon **block_jacobi) {
  PGO_REQUIRE_ARGS(p && x && grad);
  MI_TRY(check_point(p, x, "x"));
  MI_TRY(check_tangent(p, grad, "the gradient"));
  touch(grad);
  touch(p->Minv.get());
  MI_TRY(launch_assembly(p, PGO_MODEL, x->d, grad->d, p->Minv->d));
  p->x = x;
  p->x_serial = x->serial;
  if (hess) *hess = &p->hess;
  if (block_jacobi) *block_jacobi = p->bj.get();
  return MI_OK;
}

int mi_pgo_retract(mi_pgo *p, const mi_vec *x, const mi_vec *eta, mi_vec *y) {
  PGO_REQUIRE_ARGS(p && x && eta && y);
  MI_TRY(check_point(p, x, "x"));
  MI_TRY(check_point(p, y, "y"));
  MI_TRY(check_tangent(p, eta, "the tangent"));
  MI_REQUIRE(y->d != x->d, "the retracted point must not alias the current one");
  return launch_retract(p, x, eta, y);
}

// One trial step of a trust-region method at the point x the model is bound to (reference Riemannian/TNT.h:493-512,
// 573-585): Hess h with |h|^2, <g,h>, <h,Hess h>; x+ = retract(x, h); the gradient-only assembly at x+ with f(x+) from the
// same pass and |grad f(x+)|^2; with_precon: the gradient-and-inverse-blocks form instead and |M+^-1 grad f(x+)|^2.  ONE
// launch chain, ONE read-back; every number from the kernels, grids and summation orders of the separate calls.
int mi_pgo_trial(mi_pgo *p, const mi_vec *x, const mi_vec *h, const mi_vec *g, int with_precon, mi_vec *x_trial, double out[6]) {
  PGO_REQUIRE_ARGS(p && x && h && g && x_trial && out);
  MI_REQUIRE(bound_to(p->x, p->x_serial, x), "mi_pgo_trial: the model is not bound to this x (call mi_pgo_model first)");
  MI_TRY(check_point(p, x, "x"));
  MI_TRY(check_point(p, x_trial, "x_trial"));
  MI_TRY(check_tangent(p, h, "h"));
  MI_TRY(check_tangent(p, g, "g"));
  MI_REQUIRE(x_trial->d != x->d, "the trial point must not alias the current one");
  mi_ctx *ctx = p->ctx;
  const size_t n = 6 * p->N;
  MI_TRY(ensure_trial_arrays(p));
  ctx->fusion.fused_trial_steps++;  // (a refused call is not a step)
  MI_TRY(pgo_apply(&p->hess, h, p->Hh.get()));
  {
    const double *xs[3] = {h->d, g->d, h->d}, *ys[3] = {h->d, h->d, p->Hh->d};
    MI_TRY(dot_batch_to_slots(ctx, 3, xs, ys, n, SLOT_MISC));
  }
  MI_TRY(launch_retract(p, x, h, x_trial));
  touch(p->grad_trial.get());
  MI_TRY(launch_assembly(p, with_precon ? PGO_GRAD_PRECON : PGO_GRAD, x_trial->d, p->grad_trial->d,
                         with_precon ? p->Minv_trial->d : nullptr));
  MI_TRY(rows_to_slot(p, ctx->scalars + SLOT_MISC + 3));
  {
    const double *gn[1] = {p->grad_trial->d};
    MI_TRY(dot_batch_to_slots(ctx, 1, gn, gn, n, SLOT_MISC + 4));
  }
  if (with_precon) {
    MI_TRY(mi_precon_apply(p->bj_trial.get(), p->grad_trial.get(), p->Pg.get()));
    const double *xs[1] = {p->Pg->d};
    MI_TRY(dot_batch_to_slots(ctx, 1, xs, xs, n, SLOT_MISC + 5));
  }
  static_assert(SLOT_MISC + 6 <= SLOT_GDIR, "slot map");
  double buf[6];
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, with_precon ? 6 : 5, buf));  // the one read-back
  out[0] = .25 * buf[3];
  out[1] = buf[0];
  out[2] = buf[1];
  out[3] = buf[2];
  out[4] = buf[4];
  out[5] = with_precon ? buf[5] : -1.0;
  return MI_OK;
}

// Host only, no device: the layout pgo_pack builds for the problem, from ONE run of the packer.  counts = {N, E, nslices,
// nnzb, padded}; arrays 0 ... 7 = slice_ptr (long long), perm, nbr (int), slot (uint32_t), rinc, tinc, kinc, tauinc (double):
// n[a] receives the number of elements of array a, and up to cap[a] of them are copied to out[a].  out may be null (sizes
// only: then cap is not read).
int mi_debug_pgo_pack(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *tt,
                      const double *kappa, const double *tau, size_t counts[5], void *const out[8], const size_t cap[8],
                      size_t n[8]) {
  MI_REQUIRE(counts && n && (E == 0 || (ei && ej && Rt && tt && kappa && tau)) && (!out || cap), "null argument");
  PgoPack P;
  std::string err;
  MI_REQUIRE(pgo_pack(N, E, ei, ej, Rt, tt, kappa, tau, P, err) == 0, "%s", err.c_str());
  counts[0] = P.N, counts[1] = P.E, counts[2] = P.nslices, counts[3] = P.nnzb, counts[4] = P.padded;
  const void *src[8] = {P.slice_ptr.data(), P.perm.data(), P.nbr.data(), P.slot.data(),
                        P.rinc.data(), P.tinc.data(), P.kinc.data(), P.tauinc.data()};
  const size_t len[8] = {P.slice_ptr.size(), P.perm.size(), P.nbr.size(), P.slot.size(),
                         P.rinc.size(), P.tinc.size(), P.kinc.size(), P.tauinc.size()};
  const size_t width[8] = {sizeof(long long), sizeof(int), sizeof(int), sizeof(uint32_t),
                           sizeof(double), sizeof(double), sizeof(double), sizeof(double)};
  for (int a = 0; a < 8; ++a) {
    n[a] = len[a];
    if (!out || !out[a]) continue;
    const size_t m = std::min(len[a], cap[a]);
    if (m > 0) std::memcpy(out[a], src[a], m * width[a]);
  }
  return MI_OK;
}

// The three curvature sums of ONE fused pass, as STPCG's consumers see them: h = H eta through k_pgo_hvp<true> (ungated),
// its workgroup partial rows reduced in row order; out = {<eta,h>, <h,h>, <eta,eta>}.  The model must have been assembled.
// Sync.
int mi_debug_pgo_hvp_dots(mi_pgo *p, const mi_vec *eta, mi_vec *h, double out[3]) {
  PGO_REQUIRE_ARGS(p && eta && h && out);
  MI_TRY(check_tangent(p, eta, "eta"));
  MI_TRY(check_tangent(p, h, "h"));
  MI_REQUIRE(eta->d != h->d, "operator input and output must not alias");
  MI_REQUIRE(p->x != nullptr, "mi_debug_pgo_hvp_dots: no model has been assembled");
  mi_ctx *ctx = p->ctx;
  touch(h);
  int rows = 0;
  MI_TRY(pgo_apply_common(&p->hess, eta, h, true, &rows, /*gated=*/false));
  MI_TRY(reduce_rows_allreduce(ctx, ctx->partials, rows, 3, ctx->scalars + SLOT_MISC));
  return read_slots_sync(ctx, SLOT_MISC, 3, out);
}

// What the last mi_pgo_model wrote, downloaded (sync).  which = 0: Bblk, 1: Gblk (padded * 9 each), 2: Nsl (nslices * 19 * 64),
// 3: Minv (18N), 4: the inverse blocks the last mi_pgo_trial with with_precon left at its trial point (18N).
// info (may be null) = {nslices, nnzb, padded, workgroups of the assembly}.  *count as in mi_debug_pgo_pack.
int mi_debug_pgo_blocks(mi_pgo *p, int which, double *out, size_t cap, size_t *count, size_t info[4]) {
  PGO_REQUIRE_ARGS(p && count && (out || cap == 0));
  if (info) info[0] = p->nslices, info[1] = p->nnzb, info[2] = p->padded, info[3] = (size_t)model_grid(p);
  const double *src = nullptr;
  size_t n = 0;
  switch (which) {
    case 0: src = p->Bblk.get(), n = p->padded * 9; break;
    case 1: src = p->Gblk.get(), n = p->padded * 9; break;
    case 2: src = p->Nsl.get(), n = p->nslices * kNodeComps * 64; break;
    case 3: src = p->Minv->d, n = 18 * p->N; break;
    case 4:
      MI_REQUIRE(p->Minv_trial != nullptr, "no trial step has been taken");
      src = p->Minv_trial->d, n = 18 * p->N;
      break;
    default: MI_REQUIRE(false, "mi_debug_pgo_blocks: which must lie in [0, 4]");
  }
  *count = n;
  const size_t m = std::min(n, cap);
  if (m > 0) {
    MI_TRY(stream_wait(p->ctx, "mi_debug_pgo_blocks"));
    MI_HIP(hipMemcpy(out, src, m * sizeof(double), hipMemcpyDeviceToHost));
  }
  return MI_OK;
}

}  // extern "C"
