// so3.hip -- chordal rotation averaging on SO(3)^N (BASELINE cfg3):
//     f(R) = 1/2 sum_e w_e | R_j - R_i Rt_e |_F^2 ,  e = (i -> j)
// as device callables for TNT (Objective, QuadraticModel, Retraction; metric = coordinate dot).
// The reference has no manifold code beyond S^2 (tests/TNT_unit_test.cpp:73-117); problem definition
// and formulas are shared with the CPU oracle (oracle/problems.c, "SO(3)^N"):
//     tangent at R_i: R_i hat(xi_i), xi in R^3;  grad_i = vee(Q_i - Q_i'),  Q_i = R_i' (L R)_i
//     Hess[xi]_i = vee(T_i - T_i'),  T_i = R_i' (L V)_i - hat(xi_i) sym(Q_i),  V_i = R_i hat(xi_i)
// with L the connection Laplacian.  Hess is LINEAR in xi with 3x3 blocks, so the quadratic model is
// assembled ONCE per outer iteration as a symmetric 3x3-block sparse matrix
//     h_i = D_i xi_i - sum_{inc (i,j)} w B_ij xi_j ,   D_i = 2 degw_i I - (tr(C_i) I - C_i),  C_i = sym(Q_i)
// and every STPCG pass is ONE kernel: block-ELL SpMV fused with the three curvature inner products
// <xi,h>, <h,h>, <xi,xi> (IterativeSolvers.h:300,305-306).  D_i^-1 is the 3x3 block-Jacobi
// preconditioner (fused into k_cg_update, PRE_BLOCK3).
//
// Layout: incidences in SELL-64-sigma over nodes (sigma = 1024: nodes degree-sorted inside each
// workgroup window, perm[slice*64+lane] = node); block component c of entry (slice s, k, lane) at
// ((slice_ptr[s] + k) * 9 + c) * 64 + lane  => each of the 9 component streams is coalesced; the
// diagonal blocks D_i are kept in the same slice order (Dsl).
// Algorithmic bytes per HVP: 72 (nnzb + N) + 4 nnzb + 8 (3N read + 3N written)  [nnzb = incidences].
//
// The same problem as a nonlinear least-squares one for TNLS / LSQR (mi_so3n_residual, mi_so3n_jacobian):
//     F(R)_e = sqrt(w_e) (R_j - R_i Rt_e)  in R^{9E},   f = 1/2 |F|^2,   dF* F = grad f
//     (dF xi)_e = sqrt(w_e) (R_j hat(xi_j) - R_i hat(xi_i) Rt_e)
//     (dF* Y)_i = sum_{incidences of i, slot order} -sqrt(w_e) vee(R_i' Y_e Rt_e') [i first node of e] / +sqrt(w_e) vee(R_i' Y_e)
// F and dF walk the EDGES in the caller's order (one thread per edge: per-edge streams of the end points, sqrt(w) and the
// measurement -- a quaternion when the problem is SQ), dF* walks the node-centric SELL incidence layout above (one lane per
// node, its incidences summed in slot order: no atomics) with one 4-byte word per slot, edge << 1 | (node is the first
// node of the edge); the measurement a first node needs, Rt_e', is what Sinc holds for that slot already.
// How the rotations reach the Jacobian kernels: RANDOM GATHERS from a buffer of the Jacobian's own (Jrot), written once per
// linearisation -- the 32-byte quaternion records copied from Rq when they are valid for the point (mi_so3n::rq), else
// the 72-byte rows copied from R.  A per-edge stream of both end rotations would be 64 (144) coalesced bytes per edge per
// application from HBM, written as 2E records per linearisation; the node buffer is 32 N bytes (16 MB at N = 5e5) that the
// 2E gathers of a pass re-visit out of L2 / MALL, and dF* needs only the lane's own rotation.  The buffer is also what keeps
// the operators valid while TNLS evaluates F at trial points: nothing else writes it.
// Algorithmic bytes per application [quaternion forms; (matrix forms)], E edges, nnzb = 2E:
//     F      16 E (end points, sqrt w) + 32 (72) E measurement + 64 (144) E rotations + 72 E written           = 184 (304) E
//     dF     the same reads + 48 E (xi_i, xi_j) + 72 E written [+ 72 E read: apply_sub_scaled]                  = 232 (352) E [+ 72 E]
//     dF*    nnzb (8 weight + 4 word + 72 Y_e) + 32 (72) E measurement at first nodes + N (4 + 32 (72) + 24 written [+ 24])
//                                                                                                               = 200 (240) E + 60 (100) N [+ 24 N]
#include <algorithm>

#include "mi_internal.h"
#include "so3_pack.h"
#include "so3_round.h"

using namespace mi;

namespace {

constexpr bool kBsr3NtDefault = true;  // 123.5 -> 112.3 us per block-Jacobi step at N = 5e5 (r03)

struct IncView {
  size_t N, nslices;
  const long long *__restrict__ slice_ptr;
  const int *__restrict__ perm;   // node owned by (slice, lane), -1 for the padding lanes of the last window
  const int *__restrict__ nbr;    // neighbour node j (padding: own node)
  // (padding entries carry weight 0 in winc, which is what the kernels test: the edge ids and the head/tail flags the
  // packing uses stay on the host, 4 + 1 bytes per incidence entry nobody streams -- until the Jacobian is first asked
  // for: mi_so3n::slot_edge, k_so3_jact)
};
// the edges in the caller's order (mi_so3n_residual, mi_so3n_jacobian; uploaded on first use)
struct EdgeView {
  size_t E;
  const int2 *__restrict__ ij;     // (i, j) of e = (i -> j)
  const double *__restrict__ Se;   // measurement Rt_e, component-major: component c of edge e at c * E + e (4 or 9 components)
  const double *__restrict__ sw;   // sqrt(w_e)
};

__device__ __forceinline__ void mat3_mul(const double *A, const double *B, double *C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void mat3_mul_at(const double *A, const double *B, double *C) {  // A' B
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
// M = Q hat(e_m) : column operations on Q (hat(e_m) has two non-zeros)
__device__ __forceinline__ void q_hat_basis(const double *Q, int m, double *M) {
  // hat(e0) = [0 0 0; 0 0 -1; 0 1 0], hat(e1) = [0 0 1; 0 0 0; -1 0 0], hat(e2) = [0 -1 0; 1 0 0; 0 0 0]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double q0 = Q[r * 3], q1 = Q[r * 3 + 1], q2 = Q[r * 3 + 2];
    if (m == 0) { M[r * 3] = 0; M[r * 3 + 1] = q2; M[r * 3 + 2] = -q1; }
    else if (m == 1) { M[r * 3] = -q2; M[r * 3 + 1] = 0; M[r * 3 + 2] = q0; }
    else { M[r * 3] = q1; M[r * 3 + 1] = -q0; M[r * 3 + 2] = 0; }
  }
}

// One thread per node: gradient, C_i, D_i, D_i^-1, and the off-diagonal blocks w B_ij of the Hessian.
// Sinc / winc: the measurement of every incidence as ITS node uses it (Rt_e at the head, Rt_e' at the tail) and its
// weight, in the incidences' own component-major slot order -- static, built once by mi_so3n_create.  Gathered from
// the edge arrays they were 72 bytes at a random place per incidence (1.56 cache lines on average, each edge fetched
// from both ends: ~600 MB per assembly at N = 5e5); as a stream they are 216 MB.
// r05: the OBJECTIVE rides along.  f(R) = 1/2 sum_e w_e |R_j - R_i Rt_e|^2 is 1/4 of the same sum over INCIDENCES (every
// edge is seen from both ends, |R_j - R_i Rt| = |R_i - R_j Rt'|), and the term R_i - R_j S is formed here anyway for the
// gradient: its squared norm costs 9 multiply-adds per incidence instead of an edge pass of its own with two more
// 72-byte gathers per edge (k_so3_objective: 61 us and 416 MB at the fabric per trial step at N = 5e5).  MODEL = false:
// the objective alone (mi_so3n_objective) -- the same loop, the same partial sums, the same bits.
// fpartials: one partial row per workgroup (<= kMaxRows workgroups: a workgroup walks groups of 4 slices).
// SQ (r05): the measurements are stored as unit quaternions (w, x, y, z) -- 32 instead of 72 bytes per incidence of the
// assembly's largest read stream (227 -> 101 MB at N = 5e5) -- and expanded here (12 products).  Chosen at creation, only
// when every measurement is a rotation to rounding (|S'S - I| <= 1e-13, det > 0): the expansion re-orthonormalises what it
// is given, which must not change the problem.
__device__ __forceinline__ void quat_to_mat(double w, double x, double y, double z, double *S) {
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  S[0] = 1 - 2 * (yy + zz); S[1] = 2 * (xy - wz);     S[2] = 2 * (xz + wy);
  S[3] = 2 * (xy + wz);     S[4] = 1 - 2 * (xx + zz); S[5] = 2 * (yz - wx);
  S[6] = 2 * (xz - wy);     S[7] = 2 * (yz + wx);     S[8] = 1 - 2 * (xx + yy);
}
// Rotation -> unit quaternion (w, x, y, z), Shepperd's branch on the largest of trace, R00, R11, R22 (no cancellation in
// the pivot), contraction off: the retraction's fused form and the conversion pass below must give the same bits for
// the same matrix whatever kernel they are inlined into.
__device__ __forceinline__ void mat_to_quat(const double *R, double *q) {
#pragma clang fp contract(off)
  const double tr = R[0] + R[4] + R[8];
  double w, x, y, z;
  if (tr > 0) {
    const double s = sqrt(tr + 1.0) * 2;  // 4 w
    w = .25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2;  // 4 x
    w = (R[7] - R[5]) / s; x = .25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2;  // 4 y
    w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = .25 * s; z = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2;  // 4 z
    w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = .25 * s;
  }
  const double nrm = sqrt(w * w + x * x + y * y + z * z);
  q[0] = w / nrm; q[1] = x / nrm; q[2] = y / nrm; q[3] = z / nrm;
}
// Rq[4 i ...] = quaternion of R_i (r06): the 32-byte gather record of the model assembly
__global__ __launch_bounds__(256) void k_so3_quat(size_t N, const double *__restrict__ R, double *__restrict__ Rq) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
    double Ri[9], q[4];
#pragma unroll
    for (int c = 0; c < 9; ++c) Ri[c] = R[9 * i + c];
    mat_to_quat(Ri, q);
    *reinterpret_cast<double2 *>(Rq + 4 * i) = make_double2(q[0], q[1]);
    *reinterpret_cast<double2 *>(Rq + 4 * i + 2) = make_double2(q[2], q[3]);
  }
}
// GQ (r06): the neighbour's rotation R_j is gathered as its unit quaternion from Rq (32 bytes, never
// across a 128-byte line; two 16-byte loads) and expanded, instead of as nine doubles at a 72-byte stride (1.56 lines on
// average).  Rq is written by the retraction of the trial step (k_so3_retract<true>) or, for a point the library did not
// produce, by k_so3_quat right before the assembly.  The own rotation R_i is read from R itself.
// FORM: what the incidence loop leaves behind.  SO3_OBJECTIVE: the objective partial only; SO3_MODEL: gradient, Hessian
// blocks, diagonal blocks and their inverses; SO3_GRAD: the gradient only (GradientDescent: mi_so3n_gradient,
// mi_so3n_armijo_trial) -- the same EG / facc / degw accumulation in the same order, without Q = R_i' R_j, the three
// q_hat_basis columns, Bblk, Dsl and Dinv (72 bytes per incidence slot and 144 + 72 bytes per node that nobody reads).
enum { SO3_OBJECTIVE = 0, SO3_MODEL = 1, SO3_GRAD = 2 };
template <int FORM, bool SQ, bool GQ>
__device__ __forceinline__ void so3_model_slice(const IncView &inc, const double *__restrict__ R,
                                                const double *__restrict__ Rq,
                                                const double *__restrict__ Sinc, const double *__restrict__ winc,
                                                double *__restrict__ grad, double *__restrict__ Dinv,
                                                double *__restrict__ Bblk, double *__restrict__ Dsl, size_t slice,
                                                int lane, double &facc) {
  if (slice >= inc.nslices) return;
  const int node = inc.perm[slice * 64 + lane];
  const bool live = node >= 0;
  const size_t i = live ? (size_t)node : 0;
  double Ri[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) Ri[c] = live ? R[9 * i + c] : (c % 4 == 0 ? 1.0 : 0.0);
  double EG[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double degw = 0;
  const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
  for (long long k = b0; k < b1; ++k) {
    const size_t e0 = (size_t)k * 64 + lane;
    const double we = winc[e0];
    double Bk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live && we != 0) {
      const size_t j = (size_t)inc.nbr[e0];
      double S[9], Rj[9];
      if (GQ) {
        const double2 qa = *reinterpret_cast<const double2 *>(Rq + 4 * j), qb = *reinterpret_cast<const double2 *>(Rq + 4 * j + 2);
        quat_to_mat(qa.x, qa.y, qb.x, qb.y, Rj);
      } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) Rj[c] = R[9 * j + c];
      }
      // head: term R_i - R_j Rt (j = tail); tail: R_i - R_j Rt'  (the transposition is in Sinc)
      if (SQ) {
        const double *sq = Sinc + (size_t)k * 4 * 64 + lane;
        quat_to_mat(sq[0], sq[64], sq[128], sq[192], S);
      } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) S[c] = Sinc[((size_t)k * 9 + c) * 64 + lane];
      }
      double RjS[9];
      mat3_mul(Rj, S, RjS);
      double q = 0;
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const double d = Ri[c] - RjS[c];
        EG[c] += we * d;
        q += d * d;
      }
      facc += we * q;
      degw += we;
      if (FORM != SO3_MODEL) continue;
      double Q[9];
      mat3_mul_at(Ri, Rj, Q);  // R_i' R_j
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double M[9], MS[9], col[3];
        q_hat_basis(Q, m, M);
        mat3_mul(M, S, MS);
        vee_skew2(MS, col);
        Bk[0 * 3 + m] = we * col[0];
        Bk[1 * 3 + m] = we * col[1];
        Bk[2 * 3 + m] = we * col[2];
      }
    }
    if (FORM == SO3_MODEL) {
#pragma unroll
      for (int c = 0; c < 9; ++c) Bblk[((size_t)k * 9 + c) * 64 + lane] = Bk[c];
    }
  }
  if (FORM == SO3_OBJECTIVE) return;
  if (!live) {
    if (FORM == SO3_MODEL) {
#pragma unroll
      for (int c = 0; c < 9; ++c) Dsl[(slice * 9 + c) * 64 + lane] = 0.0;
    }
    return;
  }
  double Q[9], C[9];
  mat3_mul_at(Ri, EG, Q);
  vee_skew2(Q, grad + 3 * i);
  if (FORM == SO3_GRAD) return;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) C[a * 3 + b] = .5 * (Q[a * 3 + b] + Q[b * 3 + a]);
  const double tr = C[0] + C[4] + C[8], d = 2 * degw - tr;
  const double a = d + C[0], b = C[1], c = C[2], e = d + C[4], f = C[5], g = d + C[8];
  // (the block is kept component-major per slice only, for the coalesced SpMV stream: a second, node-ordered copy --
  // nine scattered 8-byte stores per node, read by nobody -- was written here until late r03)
  {
    const double dd[9] = {a, b, c, b, e, f, c, f, g};
#pragma unroll
    for (int q = 0; q < 9; ++q) Dsl[(slice * 9 + q) * 64 + lane] = dd[q];
  }
  const double c00 = e * g - f * f, c01 = c * f - b * g, c02 = b * f - c * e;
  const double c11 = a * g - c * c, c12 = b * c - a * f, c22 = a * e - b * b;
  const double det = a * c00 + b * c01 + c * c02;
  double *Di = Dinv + 9 * i;
  Di[0] = c00 / det; Di[1] = c01 / det; Di[2] = c02 / det;
  Di[3] = c01 / det; Di[4] = c11 / det; Di[5] = c12 / det;
  Di[6] = c02 / det; Di[7] = c12 / det; Di[8] = c22 / det;
}

template <bool MODEL, bool SQ, bool GQ>
__global__ __launch_bounds__(256) void k_so3_model(IncView inc, const double *__restrict__ R, const double *__restrict__ Rq,
                                                   const double *__restrict__ Sinc, const double *__restrict__ winc,
                                                   double *__restrict__ grad,
                                                   double *__restrict__ Dinv, double *__restrict__ Bblk,
                                                   double *__restrict__ Dsl, double *__restrict__ fpartials) {
  __shared__ double flds[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double facc = 0;
  const size_t ngroups = (inc.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x)
    so3_model_slice<MODEL ? SO3_MODEL : SO3_OBJECTIVE, SQ, GQ>(inc, R, Rq, Sinc, winc, grad, Dinv, Bblk, Dsl, grp * 4 + w, lane, facc);
  // the workgroup's partial of the objective: workgroup b -> row b % kMaxRows of component b / kMaxRows (one workgroup
  // per group of slices keeps the dynamic balance of ~2000 short workgroups: a grid capped at kMaxRows rows cost the
  // assembly 30 us at N = 5e5); the components are added in fixed order by k_sum_slots
  facc = wave_reduce_sum(facc);
  if (lane == 0) flds[w] = facc;
  __syncthreads();
  if (threadIdx.x == 0) {
    fpartials[(size_t)(blockIdx.x / kMaxRows) * kMaxRows + blockIdx.x % kMaxRows] = (flds[0] + flds[1]) + (flds[2] + flds[3]);
    // the rows of the last component past the last workgroup read as zero (the buffer is shared with other reductions)
    const size_t total = (size_t)((gridDim.x + kMaxRows - 1) / kMaxRows) * kMaxRows, z = (size_t)gridDim.x + blockIdx.x;
    if (z < total) fpartials[z] = 0.0;
  }
}
// The gradient-only form: grid, workgroup shape and objective partial rows of k_so3_model (see there), so that
// partial_rows_to_slot reduces f exactly as mi_so3n_objective does; the gradient bit for bit the one
// k_so3_model<true> writes.  (A kernel of its own, not a third value of MODEL: the existing instantiations keep their
// names and their code.  The lines around the slice walk are repeated here on purpose: as one inlined function shared with
// k_so3_model they compile to other register counts in the 9-component-measurement forms -- k_so3_model<true, false,
// false> 166 -> 172 VGPRs, 3 -> 2 waves per SIMD)
template <bool SQ, bool GQ>
__global__ __launch_bounds__(256) void k_so3_grad(IncView inc, const double *__restrict__ R, const double *__restrict__ Rq,
                                                  const double *__restrict__ Sinc, const double *__restrict__ winc,
                                                  double *__restrict__ grad, double *__restrict__ fpartials) {
  __shared__ double flds[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double facc = 0;
  const size_t ngroups = (inc.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x)
    so3_model_slice<SO3_GRAD, SQ, GQ>(inc, R, Rq, Sinc, winc, grad, nullptr, nullptr, nullptr, grp * 4 + w, lane, facc);
  facc = wave_reduce_sum(facc);
  if (lane == 0) flds[w] = facc;
  __syncthreads();
  if (threadIdx.x == 0) {
    fpartials[(size_t)(blockIdx.x / kMaxRows) * kMaxRows + blockIdx.x % kMaxRows] = (flds[0] + flds[1]) + (flds[2] + flds[3]);
    const size_t total = (size_t)((gridDim.x + kMaxRows - 1) / kMaxRows) * kMaxRows, z = (size_t)gridDim.x + blockIdx.x;
    if (z < total) fpartials[z] = 0.0;
  }
}
// dst[0] = src[0] + ... + src[k-1] in index order (one thread)
__global__ void k_sum_slots(const double *__restrict__ src, int k, double *__restrict__ dst) {
  double s = 0;
  for (int i = 0; i < k; ++i) s += src[i];
  dst[0] = s;
}

// h = D xi - sum B_ij xi_j, fused with the three curvature dots (one 256-thread workgroup = 4 slices)
// NT: the matrix streams (diagonal blocks, off-diagonal blocks, neighbour indices -- read exactly once per pass) are
// loaded with the non-temporal policy, so that they do not evict the 12 MB of xi that the random chord gathers re-visit
// from the XCD's 4 MB L2 (A/B switch MI355OPT_BSR3_NT, measured in DESIGN 5.1).
template <bool NT>
__device__ __forceinline__ double ld_stream(const double *p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT>
__device__ __forceinline__ int ld_stream(const int *p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool DOTS, bool NT>
__global__ __launch_bounds__(kBlock) void k_bsr3_spmv(IncView inc, const CgState *__restrict__ st,
                                                      const double *__restrict__ Dsl,
                                                      const double *__restrict__ Bblk,
                                                      const double *__restrict__ xi, double *__restrict__ h,
                                                      double *__restrict__ partials) {
  __shared__ double lds[3 * kWaves];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double a[3] = {0, 0, 0};
  const size_t ngroups = (inc.nslices + kWaves - 1) / kWaves;
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t g0 = (ngroups * lb) / nb, g1 = (ngroups * (lb + 1)) / nb;
  for (size_t g = g0; g < g1; ++g) {
    const size_t slice = g * kWaves + w;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    if (node < 0) continue;
    const size_t i = (size_t)node;  // degree-sorted inside the workgroup's 1024-node window
    const double x0 = xi[3 * i], x1 = xi[3 * i + 1], x2 = xi[3 * i + 2];
    const double *D = Dsl + slice * 9 * 64 + lane;
    double h0 = ld_stream<NT>(D) * x0 + ld_stream<NT>(D + 64) * x1 + ld_stream<NT>(D + 128) * x2;
    double h1 = ld_stream<NT>(D + 192) * x0 + ld_stream<NT>(D + 256) * x1 + ld_stream<NT>(D + 320) * x2;
    double h2 = ld_stream<NT>(D + 384) * x0 + ld_stream<NT>(D + 448) * x1 + ld_stream<NT>(D + 512) * x2;
    const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
    for (long long k = b0; k < b1; ++k) {
      const size_t e0 = (size_t)k * 64 + lane;
      const size_t j = (size_t)ld_stream<NT>(inc.nbr + e0);
      const double y0 = xi[3 * j], y1 = xi[3 * j + 1], y2 = xi[3 * j + 2];
      const double *B = Bblk + (size_t)k * 9 * 64 + lane;
      h0 -= ld_stream<NT>(B) * y0 + ld_stream<NT>(B + 64) * y1 + ld_stream<NT>(B + 128) * y2;
      h1 -= ld_stream<NT>(B + 192) * y0 + ld_stream<NT>(B + 256) * y1 + ld_stream<NT>(B + 320) * y2;
      h2 -= ld_stream<NT>(B + 384) * y0 + ld_stream<NT>(B + 448) * y1 + ld_stream<NT>(B + 512) * y2;
    }
    h[3 * i] = h0; h[3 * i + 1] = h1; h[3 * i + 2] = h2;
    if (DOTS) {
      a[0] += x0 * h0; a[0] += x1 * h1; a[0] += x2 * h2;
      a[1] += h0 * h0; a[1] += h1 * h1; a[1] += h2 * h2;
      a[2] += x0 * x0; a[2] += x1 * x1; a[2] += x2 * x2;
    }
  }
  if (DOTS) block_partials_store<3>(a, lds, partials);
}

// Y_i = R_i exp(hat(xi_i))  (Rodrigues; same series switch as oracle/problems.c: orc_so3_exp)
// (80 scalar registers: see stpcg.hip, k_cg_update_s80)
// WQ (r06): also the quaternion of every Y_i into Yq (the model assembly's gather record at the trial point)
template <bool WQ>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(80))) void k_so3_retract(size_t N, const double *__restrict__ R,
                                                        const double *__restrict__ xi, double *__restrict__ Y,
                                                        double *__restrict__ Yq) {
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
    const double x0 = xi[3 * i], x1 = xi[3 * i + 1], x2 = xi[3 * i + 2];
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
    for (int c = 0; c < 9; ++c) Ri[c] = R[9 * i + c];
    mat3_mul(Ri, Ex, Yi);
#pragma unroll
    for (int c = 0; c < 9; ++c) Y[9 * i + c] = Yi[c];
    if (WQ) {
      double q[4];
      mat_to_quat(Yi, q);
      *reinterpret_cast<double2 *>(Yq + 4 * i) = make_double2(q[0], q[1]);
      *reinterpret_cast<double2 *>(Yq + 4 * i + 2) = make_double2(q[2], q[3]);
    }
  }
}

// ---- nonlinear least-squares view: F, dF, dF* (see the file header) ---------------------------------------------------
// rotation `i` of a node buffer: GQ -- 32-byte unit quaternion records (Rq layout), else 72-byte row-major rows
template <bool GQ>
__device__ __forceinline__ void load_rot(const double *__restrict__ rot, size_t i, double *Ri) {
  if (GQ) {
    const double2 qa = *reinterpret_cast<const double2 *>(rot + 4 * i), qb = *reinterpret_cast<const double2 *>(rot + 4 * i + 2);
    quat_to_mat(qa.x, qa.y, qb.x, qb.y, Ri);
  } else {
#pragma unroll
    for (int c = 0; c < 9; ++c) Ri[c] = rot[9 * i + c];
  }
}
template <bool SQ>
__device__ __forceinline__ void load_edge_meas(const EdgeView &ev, size_t e, double *S) {
  if (SQ) {
    quat_to_mat(ev.Se[e], ev.Se[ev.E + e], ev.Se[2 * ev.E + e], ev.Se[3 * ev.E + e], S);
  } else {
#pragma unroll
    for (int c = 0; c < 9; ++c) S[c] = ev.Se[(size_t)c * ev.E + e];
  }
}
// M = Q hat(x): row r of Q crossed with x
__device__ __forceinline__ void q_hat(const double *Q, double x0, double x1, double x2, double *M) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double q0 = Q[r * 3], q1 = Q[r * 3 + 1], q2 = Q[r * 3 + 2];
    M[r * 3] = q1 * x2 - q2 * x1;
    M[r * 3 + 1] = q2 * x0 - q0 * x2;
    M[r * 3 + 2] = q0 * x1 - q1 * x0;
  }
}
constexpr int kNlsBlock = 256;  // one thread per edge / per node lane, <= kMaxRows workgroups (grid-stride beyond): one
                                // partial row of the squared norm per workgroup, component 0
// F_e = sqrt(w_e) (R_j - R_i Rt_e) ; partial |F|^2
template <bool SQ, bool GQ>
__global__ __launch_bounds__(kNlsBlock) void k_so3_residual(EdgeView ev, const double *__restrict__ rot,
                                                            double *__restrict__ F, double *__restrict__ partials) {
  __shared__ double lds[4];
  double acc[1] = {0};
  const size_t stride = (size_t)gridDim.x * kNlsBlock;
  for (size_t e = (size_t)blockIdx.x * kNlsBlock + threadIdx.x; e < ev.E; e += stride) {
    const int2 ij = ev.ij[e];
    const double sw = ev.sw[e];
    double Ri[9], Rj[9], S[9], RiS[9];
    load_rot<GQ>(rot, (size_t)ij.x, Ri);
    load_rot<GQ>(rot, (size_t)ij.y, Rj);
    load_edge_meas<SQ>(ev, e, S);
    mat3_mul(Ri, S, RiS);
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const double f = sw * (Rj[c] - RiS[c]);
      F[9 * e + c] = f;
      acc[0] += f * f;
    }
  }
  block_partials_store_nw<1, kNlsBlock / 64>(acc, lds, partials);
}
// y_e = sqrt(w_e) (R_j hat(xi_j) - R_i hat(xi_i) Rt_e).  FUSED (mi_op::apply_sub_scaled, IterativeSolvers.h:707):
// y_e = that - (*scale) y_e with the partial rows of |y|^2; nothing when *mode != 0 or (gate && !*gate).
template <bool FUSED, bool SQ, bool GQ>
__global__ __launch_bounds__(kNlsBlock) void k_so3_jac(EdgeView ev, const double *__restrict__ rot,
                                                       const double *__restrict__ xi, double *__restrict__ y,
                                                       const double *__restrict__ scale, const int *__restrict__ mode,
                                                       const int *__restrict__ gate, double *__restrict__ partials) {
  __shared__ double lds[4];
  double alpha = 0;
  if (FUSED) {
    if (*mode != 0 || (gate && !*gate)) return;
    alpha = *scale;
  }
  double acc[1] = {0};
  const size_t stride = (size_t)gridDim.x * kNlsBlock;
  for (size_t e = (size_t)blockIdx.x * kNlsBlock + threadIdx.x; e < ev.E; e += stride) {
    const int2 ij = ev.ij[e];
    const size_t i = (size_t)ij.x, j = (size_t)ij.y;
    const double sw = ev.sw[e];
    double Ri[9], Rj[9], S[9], A[9], B[9], BS[9];
    load_rot<GQ>(rot, i, Ri);
    load_rot<GQ>(rot, j, Rj);
    load_edge_meas<SQ>(ev, e, S);
    q_hat(Rj, xi[3 * j], xi[3 * j + 1], xi[3 * j + 2], A);
    q_hat(Ri, xi[3 * i], xi[3 * i + 1], xi[3 * i + 2], B);
    mat3_mul(B, S, BS);
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      double t = sw * (A[c] - BS[c]);
      if (FUSED) {
        t = t - alpha * y[9 * e + c];
        acc[0] += t * t;
      }
      y[9 * e + c] = t;
    }
  }
  if (FUSED) block_partials_store_nw<1, kNlsBlock / 64>(acc, lds, partials);
}
// x_i = vee(R_i' G_i),  G_i = sum over the incidence slots of node i, in slot order, of  -sqrt(w) Y_e Rt_e'  (i the first
// node of e; Rt_e' = the slot's Sinc) or +sqrt(w) Y_e (the second).  One lane per node, 4 slices per workgroup, the walk of
// k_so3_model.  FUSED (IterativeSolvers.h:712): x_i = that - (*scale) x_i with the partial rows of |x|^2, gated as above.
template <bool FUSED, bool SQ, bool GQ>
__global__ __launch_bounds__(kNlsBlock) void k_so3_jact(IncView inc, const double *__restrict__ rot,
                                                        const double *__restrict__ Sinc, const double *__restrict__ winc,
                                                        const uint32_t *__restrict__ slot_edge,
                                                        const double *__restrict__ Y, double *__restrict__ x,
                                                        const double *__restrict__ scale, const int *__restrict__ mode,
                                                        const int *__restrict__ gate, double *__restrict__ partials) {
  __shared__ double lds[4];
  double beta = 0;
  if (FUSED) {
    if (*mode != 0 || (gate && !*gate)) return;
    beta = *scale;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[1] = {0};
  const size_t ngroups = (inc.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const size_t slice = grp * 4 + w;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    if (node < 0) continue;
    const size_t i = (size_t)node;
    double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
    for (long long k = b0; k < b1; ++k) {
      const size_t e0 = (size_t)k * 64 + lane;
      const double we = winc[e0];
      if (we == 0) continue;
      const uint32_t code = slot_edge[e0];
      const size_t e = (size_t)(code >> 1);
      const double sw = sqrt(we);
      double Ye[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) Ye[c] = Y[9 * e + c];
      if (code & 1u) {
        double S[9], YS[9];
        if (SQ) {
          const double *sq = Sinc + (size_t)k * 4 * 64 + lane;
          quat_to_mat(sq[0], sq[64], sq[128], sq[192], S);
        } else {
#pragma unroll
          for (int c = 0; c < 9; ++c) S[c] = Sinc[((size_t)k * 9 + c) * 64 + lane];
        }
        mat3_mul(Ye, S, YS);
#pragma unroll
        for (int c = 0; c < 9; ++c) G[c] -= sw * YS[c];
      } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) G[c] += sw * Ye[c];
      }
    }
    double Ri[9], Q[9], o[3];
    load_rot<GQ>(rot, i, Ri);
    mat3_mul_at(Ri, G, Q);
    vee_skew2(Q, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double t = o[c];
      if (FUSED) {
        t = t - beta * x[3 * i + c];
        acc[0] += t * t;
      }
      x[3 * i + c] = t;
    }
  }
  if (FUSED) block_partials_store_nw<1, kNlsBlock / 64>(acc, lds, partials);
}

// ---- robust loss by edge reweighting (mi_so3n_reweight) ---------------------------------------------------
//     w_e = w0_e phi(r_e),  r_e = |R_j - R_i Rt_e|_F (unweighted),  s = r_e^2 / c^2,  rho' = r phi
//     L2: phi = 1, rho = r^2 / 2;  Huber: phi = 1 | c / r, rho = r^2 / 2 | c r - c^2 / 2 (r <= c | r > c);
//     Cauchy: phi = 1 / (1 + s), rho = (c^2 / 2) log1p(s);  Geman-McClure: phi = 1 / (1 + s)^2, rho = (r^2 / 2) / (1 + s)
// k_so3_edge_weight: one thread per edge in the caller's order on the grid of edge_grid(), the loaders of k_so3_residual; the
// rotations always as the 72-byte rows of R (once per robust round: one form is enough); rot == nullptr: r = 0 (L2 restoring
// the creation-time weights needs no point).  Writes w_e, sqrt(w_e) into swe when the least-squares arrays exist, and
// three partial rows per workgroup (components 0..2 of `partials`, reduced as the residual's row): sum w0 rho(r), sum w r^2 / 2,
// the number of edges with phi < 1/2.  No atomics.
// Algorithmic bytes: 8 E (end points) + 8 E (w0) + 32 (72) E measurement + 144 E rotations + 8 E written [+ 8 E: swe]
//                                                                                                  = 200 (240) E [+ 8 E]
enum { SO3_ROBUST_L2 = 0, SO3_ROBUST_HUBER = 1, SO3_ROBUST_CAUCHY = 2, SO3_ROBUST_GM = 3 };
template <bool SQ>
__global__ __launch_bounds__(kNlsBlock) void k_so3_edge_weight(EdgeView ev, const double *__restrict__ w0,
                                                               const double *__restrict__ rot, int kind, double c,
                                                               double *__restrict__ w, double *__restrict__ swe,
                                                               double *__restrict__ partials) {
  __shared__ double lds[3 * (kNlsBlock / 64)];
  double acc[3] = {0, 0, 0};
  const double c2 = c * c;
  const size_t stride = (size_t)gridDim.x * kNlsBlock;
  for (size_t e = (size_t)blockIdx.x * kNlsBlock + threadIdx.x; e < ev.E; e += stride) {
    double r2 = 0;
    if (rot) {
      const int2 ij = ev.ij[e];
      double Ri[9], Rj[9], S[9], RiS[9];
      load_rot<false>(rot, (size_t)ij.x, Ri);
      load_rot<false>(rot, (size_t)ij.y, Rj);
      load_edge_meas<SQ>(ev, e, S);
      mat3_mul(Ri, S, RiS);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double d = Rj[k] - RiS[k];
        r2 += d * d;
      }
    }
    double phi = 1.0, rho = .5 * r2;
    if (kind == SO3_ROBUST_HUBER) {
      const double r = sqrt(r2);
      if (r > c) {
        phi = c / r;
        rho = c * r - .5 * c2;
      }
    } else if (kind == SO3_ROBUST_CAUCHY) {
      const double s = r2 / c2;
      phi = 1.0 / (1.0 + s);
      rho = .5 * c2 * log1p(s);
    } else if (kind == SO3_ROBUST_GM) {
      const double s = r2 / c2, t = 1.0 / (1.0 + s);
      phi = t * t;
      rho = .5 * r2 * t;
    }
    const double w0e = w0[e], we = w0e * phi;
    w[e] = we;
    if (swe) swe[e] = sqrt(we);
    acc[0] += w0e * rho;
    acc[1] += we * (.5 * r2);
    acc[2] += phi < .5 ? 1.0 : 0.0;
  }
  block_partials_store_nw<3, kNlsBlock / 64>(acc, lds, partials);
}
// swe = sqrt(w): the least-squares view first asked for after a reweighting (nls_upload)
__global__ __launch_bounds__(kNlsBlock) void k_so3_sqrt_w(size_t E, const double *__restrict__ w, double *__restrict__ swe) {
  const size_t stride = (size_t)gridDim.x * kNlsBlock;
  for (size_t e = (size_t)blockIdx.x * kNlsBlock + threadIdx.x; e < E; e += stride) swe[e] = sqrt(w[e]);
}
// k_so3_inc_reweight: the per-incidence weight stream from the per-edge weights, winc[slot] = w[slot_edge[slot] >> 1], one
// lane per node on the walk of k_so3_jact.  Only OCCUPIED slots are written: a padding slot keeps its weight 0 (its word is
// 0, which reads as edge 0).  What tells them apart is static and streamed already: a padding slot's neighbour is the lane's
// own node, and no edge joins a node to itself (mi_so3n_create refuses one); the padding lanes of the last slice own no node.
// gn (nullable): the Gauss-Newton scaling 1 / sqrt(2 degw_i), each three times, degw_i summed in slot order (1 for degw_i = 0).
// Algorithmic bytes: nnzb (4 neighbour + 4 word + 8 gathered + 8 written) + 4 N [+ 24 N: gn] = 48 E + 4 N [+ 24 N]
__global__ __launch_bounds__(kNlsBlock) void k_so3_inc_reweight(IncView inc, const uint32_t *__restrict__ slot_edge,
                                                                const double *__restrict__ w, double *__restrict__ winc,
                                                                double *__restrict__ gn) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t ngroups = (inc.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const size_t slice = grp * 4 + wv;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    if (node < 0) continue;
    double degw = 0;
    const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
    for (long long k = b0; k < b1; ++k) {
      const size_t e0 = (size_t)k * 64 + lane;
      if (inc.nbr[e0] == node) continue;
      const double we = w[(size_t)(slot_edge[e0] >> 1)];
      winc[e0] = we;
      degw += we;
    }
    if (gn) {
      const double d = degw > 0 ? 1.0 / sqrt(2 * degw) : 1.0;
      gn[3 * (size_t)node] = d; gn[3 * (size_t)node + 1] = d; gn[3 * (size_t)node + 2] = d;
    }
  }
}

// ---- global-optimality certificate -----------------------------------------------------------------------
// With Y in R^{3N x 3}, Y_i = R_i', and the 3N x 3N connection Laplacian (diagonal blocks degw_i I, block (i, j) = -w_e Rt_e
// and (j, i) = -w_e Rt_e' for e = (i -> j)), f(R) = const + 1/2 tr(Y' Lap Y), and the certificate matrix at R is
//     S(R) = Lap - BlockDiag(C_i),  C_i = sym(Q_i)
//     (S v)_i = (degw_i I - C_i) v_i - sum_{inc of i, slot order} w S_inc' v_nbr
// (S_inc: what Sinc holds for the slot).  tr(Y' S Y) = 0 at every R, |S Y|_F = |skew Q|_F, and for every R' in O(3)^N
// f(R') >= f(R) + (3N / 2) min(lambda_min(S), 0): S positive semidefinite at a critical point certifies the global minimum.
// The off-diagonal blocks are the static streams Sinc / winc / nbr; only the N diagonal blocks depend on the point.
//
// k_so3_cert_diag: one lane per node, the walk, the gathers and the objective partial of k_so3_model<false, ...> (grid,
// workgroup shape and accumulation order: the bits of mi_so3n_objective), leaving per node
//   the six distinct entries (00, 01, 02, 11, 12, 22) of E_i = degw_i I - C_i in slice order (entry c of (slice, lane) at
//   (slice * 6 + c) * 64 + lane; padding lanes: 0), and row c of R_i as rows 3i .. 3i+2 of column c of the column-major
//   3N x 3 panel Yp (Y(3i + r, c) = R_i[c][r]);
// and per workgroup three partial rows: the objective sum, |Q_i - Q_i'|_F^2 and tr C_i (components of kModelComps rows
// groups each, laid out as the objective's).  A body of its own: see k_so3_grad on sharing one with k_so3_model.
constexpr int kCertComps = 8;  // == kModelComps (below): partial components per quantity
template <bool SQ, bool GQ>
__global__ __launch_bounds__(256) void k_so3_cert_diag(IncView inc, const double *__restrict__ R, const double *__restrict__ Rq,
                                                       const double *__restrict__ Sinc, const double *__restrict__ winc,
                                                       double *__restrict__ Esl, double *__restrict__ Yp,
                                                       double *__restrict__ fpartials) {
  __shared__ double flds[12];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double facc = 0, gacc = 0, tacc = 0;
  const size_t ngroups = (inc.nslices + 3) / 4, ld = 3 * inc.N;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const size_t slice = grp * 4 + w;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    const bool live = node >= 0;
    const size_t i = live ? (size_t)node : 0;
    double Ri[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) Ri[c] = live ? R[9 * i + c] : (c % 4 == 0 ? 1.0 : 0.0);
    double EG[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double degw = 0;
    const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
    for (long long k = b0; k < b1; ++k) {
      const size_t e0 = (size_t)k * 64 + lane;
      const double we = winc[e0];
      if (live && we != 0) {
        const size_t j = (size_t)inc.nbr[e0];
        double S[9], Rj[9];
        if (GQ) {
          const double2 qa = *reinterpret_cast<const double2 *>(Rq + 4 * j), qb = *reinterpret_cast<const double2 *>(Rq + 4 * j + 2);
          quat_to_mat(qa.x, qa.y, qb.x, qb.y, Rj);
        } else {
#pragma unroll
          for (int c = 0; c < 9; ++c) Rj[c] = R[9 * j + c];
        }
        if (SQ) {
          const double *sq = Sinc + (size_t)k * 4 * 64 + lane;
          quat_to_mat(sq[0], sq[64], sq[128], sq[192], S);
        } else {
#pragma unroll
          for (int c = 0; c < 9; ++c) S[c] = Sinc[((size_t)k * 9 + c) * 64 + lane];
        }
        double RjS[9];
        mat3_mul(Rj, S, RjS);
        double q = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          const double d = Ri[c] - RjS[c];
          EG[c] += we * d;
          q += d * d;
        }
        facc += we * q;
        degw += we;
      }
    }
    double *Es = Esl + slice * 6 * 64 + lane;
    if (!live) {
#pragma unroll
      for (int c = 0; c < 6; ++c) Es[c * 64] = 0.0;
      continue;
    }
    double Q[9];
    mat3_mul_at(Ri, EG, Q);
    const double c01 = .5 * (Q[1] + Q[3]), c02 = .5 * (Q[2] + Q[6]), c12 = .5 * (Q[5] + Q[7]);
    Es[0] = degw - Q[0]; Es[64] = -c01; Es[128] = -c02;
    Es[192] = degw - Q[4]; Es[256] = -c12; Es[320] = degw - Q[8];
    const double s0 = Q[7] - Q[5], s1 = Q[2] - Q[6], s2 = Q[3] - Q[1];
    gacc += 2 * (s0 * s0 + s1 * s1 + s2 * s2);
    tacc += Q[0] + Q[4] + Q[8];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) Yp[(size_t)c * ld + 3 * i + r] = Ri[3 * c + r];
  }
  facc = wave_reduce_sum(facc);
  gacc = wave_reduce_sum(gacc);
  tacc = wave_reduce_sum(tacc);
  if (lane == 0) { flds[w] = facc; flds[4 + w] = gacc; flds[8 + w] = tacc; }
  __syncthreads();
  if (threadIdx.x < 3) {
    // (the rows of each quantity laid out, and its unused rows zeroed, as k_so3_model does for the objective)
    double *part = fpartials + (size_t)threadIdx.x * kCertComps * kMaxRows;
    const double *l = flds + 4 * threadIdx.x;
    part[(size_t)(blockIdx.x / kMaxRows) * kMaxRows + blockIdx.x % kMaxRows] = (l[0] + l[1]) + (l[2] + l[3]);
    const size_t total = (size_t)((gridDim.x + kMaxRows - 1) / kMaxRows) * kMaxRows, z = (size_t)gridDim.x + blockIdx.x;
    if (z < total) part[z] = 0.0;
  }
}

// The input panel of the certificate product as up to three column blocks (mi_panel_blocks): column c is column c of
// block 0 for c < n0, column c - n0 of block 1 for c < n01, else column c - n01 of block 2 (one panel: n0 = n01 = k)
struct CertCols {
  const double *b[3];
  int n0, n01;
};
// (the expansion with contraction off: an incidence and its mirror image at the other node hold conjugate quaternions, and
// rounded products make their two expansions exact transposes of each other)
__device__ __forceinline__ void quat_to_mat_nc(double w, double x, double y, double z, double *S) {
#pragma clang fp contract(off)
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  S[0] = 1 - 2 * (yy + zz); S[1] = 2 * (xy - wz);     S[2] = 2 * (xz + wy);
  S[3] = 2 * (xy + wz);     S[4] = 1 - 2 * (xx + zz); S[5] = 2 * (yz - wx);
  S[6] = 2 * (xz - wy);     S[7] = 2 * (yz + wx);     S[8] = 1 - 2 * (xx + yy);
}
// Z = S X on column-major 3N x k panels (ld = 3N), one lane per node, 4 slices per workgroup; blockIdx.y: the pass (KC
// columns each, the last one possibly fewer), all passes in one launch as in k_spmm_colmajor_win.  An incidence's weight,
// neighbour and measurement are loaded -- and the measurement expanded -- ONCE and applied to the pass's columns: the
// matrix stream (8 + 4 + 32 (72) bytes per incidence) is amortised over KC columns, the neighbour's three rows are gathered
// per column.  Every column is summed in one fixed order with contraction off -- the diagonal block's row products left
// to right, then the incidences in slot order, each as z_r - w (S_0r y_0 + S_1r y_1 + S_2r y_2) -- so column c of Z depends
// on column c of X alone and has the same bits whatever k, KC, pass or column-block split it came from.  Weight-0 slots
// (padding, or an edge of weight 0) and padding lanes do nothing.  Z must not overlap X.
// Algorithmic bytes per application, P = ceil(k / KC) passes: P (nnzb (12 + 32 (72)) + 52 N) + 48 k N  [+ 24 k nnzb gathered]
template <int KC, bool SQ>
__global__ __launch_bounds__(256) void k_so3_cert_panel(IncView inc, const double *__restrict__ Sinc,
                                                        const double *__restrict__ winc, const double *__restrict__ Esl,
                                                        CertCols X, int k, double *__restrict__ Z) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ld = 3 * inc.N;
  const int c0 = (int)blockIdx.y * KC, nc = k - c0 < KC ? k - c0 : KC;
  const double *xc[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int cc = c0 + (c < nc ? c : 0);
    xc[c] = cc < X.n0 ? X.b[0] + (size_t)cc * ld : cc < X.n01 ? X.b[1] + (size_t)(cc - X.n0) * ld : X.b[2] + (size_t)(cc - X.n01) * ld;
  }
  const size_t ngroups = (inc.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const size_t slice = grp * 4 + w;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    if (node < 0) continue;
    const size_t i = (size_t)node;
    const double *Es = Esl + slice * 6 * 64 + lane;
    const double e00 = Es[0], e01 = Es[64], e02 = Es[128], e11 = Es[192], e12 = Es[256], e22 = Es[320];
    double z[KC][3];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      z[c][0] = z[c][1] = z[c][2] = 0;
      if (c < nc) {
        const double x0 = xc[c][3 * i], x1 = xc[c][3 * i + 1], x2 = xc[c][3 * i + 2];
        z[c][0] = e00 * x0 + e01 * x1 + e02 * x2;
        z[c][1] = e01 * x0 + e11 * x1 + e12 * x2;
        z[c][2] = e02 * x0 + e12 * x1 + e22 * x2;
      }
    }
    const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
    for (long long s = b0; s < b1; ++s) {
      const size_t e0 = (size_t)s * 64 + lane;
      const double we = winc[e0];
      if (we == 0) continue;
      const size_t j = (size_t)inc.nbr[e0];
      double S[9];
      if (SQ) {
        const double *sq = Sinc + (size_t)s * 4 * 64 + lane;
        quat_to_mat_nc(sq[0], sq[64], sq[128], sq[192], S);
      } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) S[c] = Sinc[((size_t)s * 9 + c) * 64 + lane];
      }
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (c < nc) {
          const double y0 = xc[c][3 * j], y1 = xc[c][3 * j + 1], y2 = xc[c][3 * j + 2];
          z[c][0] = z[c][0] - we * (S[0] * y0 + S[3] * y1 + S[6] * y2);
          z[c][1] = z[c][1] - we * (S[1] * y0 + S[4] * y1 + S[7] * y2);
          z[c][2] = z[c][2] - we * (S[2] * y0 + S[5] * y1 + S[8] * y2);
        }
    }
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < nc) {
        double *zc = Z + (size_t)(c0 + c) * ld + 3 * i;
        zc[0] = z[c][0]; zc[1] = z[c][1]; zc[2] = z[c][2];
      }
  }
}

// ---- spectral initialisation and SO(3) rounding ----------------------------------------------------------
// The connection Laplacian is the certificate matrix with the diagonal blocks degw_i I: k_so3_cert_panel is its panel
// product once Esl holds them.  k_so3_lap_diag: one lane per node on the walk of k_so3_cert_diag, degw_i summed from winc in
// slot order (the weights IN FORCE: after mi_so3n_reweight the reweighted Laplacian; weight-0 slots skipped as there), the
// six entries (degw, 0, 0, degw, 0, degw) into the layout of k_so3_cert_diag; padding lanes write 0.  No atomics.
// Algorithmic bytes: 8 padded + 48 * 64 nslices + 4 N
__global__ __launch_bounds__(256) void k_so3_lap_diag(IncView inc, const double *__restrict__ winc, double *__restrict__ Esl) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ngroups = (inc.nslices + 3) / 4;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const size_t slice = grp * 4 + w;
    if (slice >= inc.nslices) continue;
    const bool live = inc.perm[slice * 64 + lane] >= 0;
    double degw = 0;
    const long long b0 = inc.slice_ptr[slice], b1 = inc.slice_ptr[slice + 1];
    for (long long k = b0; k < b1; ++k) {
      const double we = winc[(size_t)k * 64 + lane];
      if (live && we != 0) degw += we;
    }
    double *Es = Esl + slice * 6 * 64 + lane;
    Es[0] = degw; Es[64] = 0.0; Es[128] = 0.0;
    Es[192] = degw; Es[256] = 0.0; Es[320] = degw;
  }
}
// Z = D^-1 X on column-major 3N x k panels (ld = 3N), D = degw_i on the three rows of node i, read from the Laplacian's
// diagonal (entry 0 of Esl, slice order): the Jacobi preconditioner of the spectral solve.  A node with degw_i = 0 copies.
// One lane per node; a true division (the bits of X / degw).  Z may be X.
__global__ __launch_bounds__(256) void k_so3_lap_jacobi(IncView inc, const double *__restrict__ Esl, int k, const double *X,
                                                        double *Z) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ngroups = (inc.nslices + 3) / 4, ld = 3 * inc.N;
  for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const size_t slice = grp * 4 + w;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    if (node < 0) continue;
    const double degw = Esl[slice * 6 * 64 + lane];
    const bool scale = degw != 0;
    const size_t r0 = 3 * (size_t)node;
    for (int c = 0; c < k; ++c) {
      const double *x = X + (size_t)c * ld + r0;
      double *z = Z + (size_t)c * ld + r0;
      const double x0 = x[0], x1 = x[1], x2 = x[2];
      z[0] = scale ? x0 / degw : x0; z[1] = scale ? x1 / degw : x1; z[2] = scale ? x2 / degw : x2;
    }
  }
}

// The four 8-byte words one rounding call leaves on the device (mi_so3n::round_words; all integer adds and order-preserving
// integer min / max: the same bits on every run):
//   [0] sum_i sign(det V_i) as a two's-complement integer (k_so3_round_sign; the panel form only)
//   [1] blocks with det < 0 as given   [2] degenerate blocks
//   [3] the bits of a double >= 0: min over the other blocks of (sigma_2 + d sigma_3) / sigma_1 (panel form) or max of
//       |M_i' M_i - I|_F (point form) -- the bit pattern of a non-negative double orders as the number does
enum { RW_SIGN = 0, RW_NEG = 1, RW_DEGENERATE = 2, RW_EXTREME = 3, RW_WORDS = 4 };
__global__ void k_so3_round_init(unsigned long long *words, unsigned long long extreme) {
  words[RW_SIGN] = 0; words[RW_NEG] = 0; words[RW_DEGENERATE] = 0; words[RW_EXTREME] = extreme;
}
// block i of the column-major 3N x 3 panel as M_i = V[3i .. 3i+2, :]' (the layout of Yp in k_so3_cert_diag), row-major
__device__ __forceinline__ void load_panel_block(const double *__restrict__ V, size_t ld, size_t i, double *M) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[3 * r + c] = V[(size_t)r * ld + 3 * i + c];
}
// the counting pass of the global sign: sum_i sign(det V_i) (0 for det = 0 or NaN) into words[RW_SIGN]
__global__ __launch_bounds__(256) void k_so3_round_sign(size_t N, const double *__restrict__ V, unsigned long long *words) {
  const size_t stride = (size_t)gridDim.x * 256, ld = 3 * N;
  double acc = 0;  // (an integer of magnitude <= N < 2^31: exact)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
    double M[9];
    load_panel_block(V, ld, i, M);
    const double det = so3_det3(M);
    acc += det > 0 ? 1.0 : det < 0 ? -1.0 : 0.0;
  }
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0 && acc != 0) atomicAdd(words + RW_SIGN, (unsigned long long)(long long)acc);
}
// R_i = the rotation nearest to M_i (so3_round.h), one lane per node, everything in registers.
// PANEL: M_i from the eigenvector panel, negated when the sign sum of k_so3_round_sign is negative (a basis that landed in
// the reflected gauge: -V spans the same space; a tie does not flip); else M_i = row-major block i of the 9N point, and
// the orthogonality defect of the input rides along.  in may be out in the point form (a lane reads its block first).
template <bool PANEL>
__global__ __launch_bounds__(256) void k_so3_round(size_t N, const double *in, double *out, unsigned long long *words) {
  const size_t stride = (size_t)gridDim.x * 256, ld = 3 * N;
  const bool flip = PANEL && (long long)words[RW_SIGN] < 0;
  double neg = 0, deg = 0, ext = PANEL ? HUGE_VAL : 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
    double M[9], Ri[9], sep, d;
    bool degenerate;
    if (PANEL) {
      load_panel_block(in, ld, i, M);
    } else {
#pragma unroll
      for (int c = 0; c < 9; ++c) M[c] = in[9 * i + c];
    }
    neg += so3_det3(M) < 0 ? 1.0 : 0.0;
    if (flip) {
#pragma unroll
      for (int c = 0; c < 9; ++c) M[c] = -M[c];
    }
    so3_nearest_rotation(M, Ri, sep, d, degenerate);
    deg += degenerate ? 1.0 : 0.0;
    if (PANEL) {
      if (!degenerate) ext = fmin(ext, sep);
    } else {
      double G[9], q = 0;
      mat3_mul_at(M, M, G);
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const double e = G[c] - (c % 4 == 0 ? 1.0 : 0.0);
        q += e * e;
      }
      if (!degenerate && q == q) ext = fmax(ext, sqrt(q));
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) out[9 * i + c] = Ri[c];
  }
  neg = wave_reduce_sum(neg);
  deg = wave_reduce_sum(deg);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(ext, off, 64);
    ext = PANEL ? fmin(ext, o) : fmax(ext, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (neg != 0) atomicAdd(words + RW_NEG, (unsigned long long)neg);
    if (deg != 0) atomicAdd(words + RW_DEGENERATE, (unsigned long long)deg);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(ext);
    if (PANEL) atomicMin(words + RW_EXTREME, bits);
    else atomicMax(words + RW_EXTREME, bits);
  }
}

}  // namespace

// The certificate matrix S(R) of mi_so3n_certificate: the problem's static incidence streams plus a copy of what depends
// on the point (the diagonal blocks E_i = degw_i I - C_i, the panel Y), written by k_so3_cert_diag and by nothing else
struct mi_so3n_cert {
  mi_so3n *q = nullptr;
  DevPtr<double> Esl;  // nslices * 6 * 64: the six distinct entries of E_i in slice order
  Owned<mi_vec> Y;     // 9N: the column-major 3N x 3 panel Y, Y_i = R_i' (null: the slot of mi_so3n_laplacian)
};
void mi::HandleDestroy::operator()(mi_so3n_cert *c) const { delete c; }

// What is below `lazily made` appears when an entry point first needs it (TNT / GradientDescent users allocate none of the
// least-squares, certificate, Laplacian or reweighting memory): who asks, what it is written from and what invalidates it
// is the table of DESIGN.md 5.1 ("Lazily made state of mi_so3n"); the ensure_* functions are its only writers.
struct mi_so3n {
  mi_ctx *ctx = nullptr;
  size_t N = 0, E = 0, nslices = 0, nnzb = 0, padded = 0;
  DevPtr<long long> slice_ptr;
  DevPtr<int> perm, nbr;
  Owned<mi_vec> Dinv;           // 9N (node order): the inverse diagonal blocks, the block-Jacobi preconditioner
  DevPtr<double> Bblk;          // padded * 9
  DevPtr<double> Sinc, winc;    // padded * 9 (or * 4: sinc_quat), padded: per-incidence measurement and weight
  bool sinc_quat = false;       // Sinc holds unit quaternions (all measurements are rotations to rounding)
  DevPtr<double> Dsl;           // nslices * 9 * 64: diagonal blocks in slice order
  DevPtr<double> Rq;            // 4 N: unit quaternions of the point the NEXT assembly gathers from (r06; null:
                                // SO3_NO_RQUAT -- the assembly gathers R itself)
  mi_op hess;
  mi_precon bj;
  const mi_vec *R = nullptr;    // the point the model is bound to (mi_so3n_model) ...
  uint64_t R_serial = 0;        // ... by handle AND serial (mi::bound_to)
  // Keys, each the handle AND the identity of its contents (mi::VecKey).  trial: the point whose whole model sits in the
  // _next arrays (mi_so3n_trial; swapped in by mi_so3n_model for the same vector); armijo: the point whose GRADIENT ONLY
  // sits in grad_next (mi_so3n_armijo_trial) -- at most one of the two is live, whoever fills grad_next drops both;
  // rq: the vector whose quaternion records Rq holds (written by the retraction of a fused trial step, cleared when the
  // assembly converts another point into Rq; mi_so3n_residual / mi_so3n_jacobian gather quaternions only then).
  VecKey trial, armijo, rq;
  // host copies kept from creation for the first-use uploads
  std::vector<int32_t> h_ij;      // 2E: (i, j) per edge
  std::vector<double> h_Se, h_w;  // E * (4 | 9) component-major measurement stream (as sinc_quat says); E weights
  std::vector<uint32_t> h_slot;   // padded: edge << 1 | (the slot's node is the first node of the edge); padding 0
  bool w_nonneg = true;
  // ---- lazily made ----
  Owned<mi_vec> grad_next;                 // 3N
  Owned<mi_vec> Dinv_next, Hh, Pg;         // the trial arrays: 9N, 3N, 3N ...
  DevPtr<double> Bblk_next, Dsl_next;      // ... and the second set of Bblk, Dsl
  DevPtr<int2> e_ij;                       // the edge streams: E ...
  DevPtr<double> Se;                       // ... E * (4 | 9)
  DevPtr<double> swe;                      // E: sqrt(w_e) of the weights in force
  DevPtr<uint32_t> slot_edge;              // the slot words: padded
  DevPtr<double> Jrot;                     // 9N: the rotations the bound dF / dF* read (4N used when jac_quat)
  bool jac_quat = false;
  mi_op dF, dFt;
  Owned<mi_vec> gn_diag;                   // 3N: 1 / sqrt(2 degw_i), each three times, of the weights in force
  Owned<mi_op> gn_op;
  Owned<mi_so3n_cert> cert;                // mi_so3n_certificate: rebound by every call
  Owned<mi_so3n_cert> lap;                 // mi_so3n_laplacian: a slot of its own (Y stays null), refreshed by every call
  DevPtr<unsigned long long> round_words;  // RW_WORDS: what mi_so3n_round / mi_so3n_project count
  DevPtr<double> w0, w_cur;                // E each: the creation-time weights and, from the first reweighting on, the
                                           // weights in force (what winc, swe and gn_diag were last written from)
};

namespace {

static_assert(kSo3Window == (size_t)kBlock, "the degree-sorted window of so3_pack.h is the workgroup pass of k_bsr3_spmv");
// workgroups of the model assembly: one per group of 4 slices while their objective partials fit 8 components of
// kMaxRows rows (N <= 2.1e6 rotations), a grid-stride walk beyond
constexpr int kModelComps = 8;
static_assert(kCertComps == kModelComps, "k_so3_cert_diag lays its partial rows out as k_so3_model does");
int model_grid(const mi_so3n *q) { return (int)std::min<size_t>((q->nslices + 3) / 4, (size_t)kModelComps * kMaxRows); }
IncView view(const mi_so3n *q) { return IncView{q->N, q->nslices, q->slice_ptr.get(), q->perm.get(), q->nbr.get()}; }
// a problem that gathers quaternions gets those of R into q->Rq (one pass over R) unless they are there already
// (have_quat: the retraction of a trial step wrote them, or the rq key says so)
void ensure_rq(mi_so3n *q, const double *R, bool have_quat) {
  if (!q->Rq || have_quat) return;
  q->rq.clear();  // (Rq is about to hold the conversion of a point given by address only)
  hipLaunchKernelGGL(k_so3_quat, dim3(grid_for(q->ctx, q->N, 1)), dim3(256), 0, q->ctx->stream, q->N, R, q->Rq.get());
}
// what was worked out at another point or with other weights: the speculative trial model, the Armijo gradient and, for a
// change of the weights, the bound model (the rq key describes a point, not the weights, and stays)
void invalidate_models(mi_so3n *q, bool also_binding) {
  q->trial.clear();
  q->armijo.clear();
  if (also_binding) q->R = nullptr, q->R_serial = 0;
}
// the assembly in one of its forms (SO3_OBJECTIVE: no outputs; SO3_GRAD: grad only), objective partials into ctx->partials2
// have_quat: see ensure_rq (a point the library did not produce -- the start, the statement sequence's calls -- is converted)
void launch_assembly(mi_so3n *q, int form, int grid, const double *R, double *grad, double *Dinv, double *Bblk, double *Dsl,
                     bool have_quat = false) {
  mi_ctx *ctx = q->ctx;
  const bool gq = q->Rq != nullptr;
  const double *Rq = q->Rq.get(), *Sinc = q->Sinc.get(), *winc = q->winc.get();
  ensure_rq(q, R, have_quat);
  DISPATCH_3(form, FORM, SO3_OBJECTIVE, SO3_MODEL, SO3_GRAD, DISPATCH_FLAG(q->sinc_quat, SQ, DISPATCH_FLAG(gq, GQ,
      if (FORM == SO3_GRAD) {
        KScope ks(ctx, MI_K_SO3_GRAD);
        hipLaunchKernelGGL((k_so3_grad<SQ, GQ>), dim3(grid), dim3(256), 0, ctx->stream, view(q), R, Rq, Sinc, winc, grad,
                           ctx->partials2);
      } else {
        hipLaunchKernelGGL((k_so3_model<FORM == SO3_MODEL, SQ, GQ>), dim3(grid), dim3(256), 0, ctx->stream, view(q), R, Rq,
                           Sinc, winc, grad, Dinv, Bblk, Dsl, ctx->partials2);
      })));
}
// quantity `which` of the partial rows a pass of `grid` workgroups left in ctx->partials2 -> one (all-reduced) sum in
// *slot.  0: the objective sum of the assembly in any of its forms and of k_so3_cert_diag; 1, 2: |Q - Q'|^2 and tr C of
// k_so3_cert_diag
int partial_rows_to_slot(mi_so3n *q, int grid, int which, double *slot) {
  mi_ctx *ctx = q->ctx;
  const double *rows = ctx->partials2 + (size_t)which * kCertComps * kMaxRows;
  const int comps = (grid + kMaxRows - 1) / kMaxRows;
  if (comps == 1) return reduce_rows_allreduce(ctx, rows, grid, 1, slot);
  // (the rows of the last component past the last workgroup were zeroed by the kernel itself)
  double *tmp = ctx->scalars + SLOT_RAW + which * kCertComps;  // (free outside mi_stiefel_gram)
  MI_TRY(reduce_rows_allreduce(ctx, rows, kMaxRows, comps, tmp));
  hipLaunchKernelGGL(k_sum_slots, dim3(1), dim3(1), 0, ctx->stream, (const double *)tmp, comps, slot);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int so3_apply_common(mi_op *self, const mi_vec *in, mi_vec *out, bool dots, int *nparts) {
  mi_so3n *q = (mi_so3n *)self->impl;
  mi_ctx *ctx = q->ctx;
  const size_t ngroups = (q->nslices + kWaves - 1) / kWaves;
  const int grid = uniform_grid(ctx, ngroups);
  KScope ks(ctx, MI_K_BSR3_SPMV_DOTS);
  constexpr bool nt = kBsr3NtDefault;
#define BSR3(DV, NTV, STATE, PART)                                                                               \
  hipLaunchKernelGGL((k_bsr3_spmv<DV, NTV>), dim3(grid), dim3(kBlock), 0, ctx->stream, view(q), STATE,          \
                     (const double *)q->Dsl.get(), (const double *)q->Bblk.get(), (const double *)in->d, out->d, PART)
  if (dots) {
    if (nt) BSR3(true, true, ctx->cg_live, ctx->partials); else BSR3(true, false, ctx->cg_live, ctx->partials);
  } else {
    if (nt) BSR3(false, true, (const CgState *)nullptr, (double *)nullptr);
    else BSR3(false, false, (const CgState *)nullptr, (double *)nullptr);
  }
#undef BSR3
  if (nparts) *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}
int so3_apply(mi_op *self, const mi_vec *in, mi_vec *out) { return so3_apply_common(self, in, out, false, nullptr); }
int so3_apply_dots(mi_op *self, const mi_vec *in, mi_vec *out, int *np) { return so3_apply_common(self, in, out, true, np); }
// v = D^-1 r by the library's block-Jacobi kernel, through a preconditioner made for the call
int block3_apply(mi_ctx *ctx, const mi_vec *Dinv, const mi_vec *r, mi_vec *v) {
  mi_precon *tmp = nullptr;
  MI_TRY(mi_precon_create_block3(ctx, Dinv, &tmp));
  const int s = mi_precon_apply(tmp, r, v);
  mi_precon_destroy(tmp);
  return s;
}
int so3_bj_apply(mi_precon *self, const mi_vec *r, mi_vec *v) {
  return block3_apply(self->ctx, ((mi_so3n *)self->impl)->Dinv.get(), r, v);
}
// an operator the problem lends out: mi_op_destroy on it is a no-op
mi_op borrowed_op(mi_ctx *ctx, size_t n_in, size_t n_out, decltype(mi_op::apply) apply,
                  decltype(mi_op::apply_sub_scaled) apply_sub_scaled, void *impl) {
  mi_op op;
  op.ctx = ctx, op.n = n_in, op.n_out = n_out, op.impl = impl, op.borrowed = true;
  op.apply = apply, op.apply_sub_scaled = apply_sub_scaled;
  return op;
}

// Y = R exp(hat xi) as a trial point: a problem that gathers quaternions gets those of Y in q->Rq from the same kernel
// (the bits k_so3_quat would give), so the assembly at Y needs no conversion pass
int retract_trial(mi_so3n *q, const mi_vec *R, const mi_vec *xi, mi_vec *Y) {
  if (!q->Rq) return mi_so3n_retract(q, R, xi, Y);
  touch(Y);
  hipLaunchKernelGGL(k_so3_retract<true>, dim3(grid_for(q->ctx, q->N, 1)), dim3(kBlock), 0, q->ctx->stream, q->N,
                     (const double *)R->d, (const double *)xi->d, Y->d, q->Rq.get());
  MI_HIP(hipGetLastError());
  q->rq.set(Y);
  return MI_OK;
}
// The tail of both trial steps: the assembly at the trial point retract_trial produced, in the given form, the gradient
// into grad_next and the other outputs where the caller says; the sum of the objective partials of the same pass,
// reduced exactly as mi_so3n_objective does, into slot f_slot; |grad f(R+)|^2 as metric(g, g) forms it (mi_vec_dot)
// into slot g2_slot
int trial_tail(mi_so3n *q, int form, const mi_vec *R_trial, double *Dinv, double *Bblk, double *Dsl, int f_slot,
               int g2_slot) {
  mi_ctx *ctx = q->ctx;
  const int grid = model_grid(q);
  launch_assembly(q, form, grid, R_trial->d, q->grad_next->d, Dinv, Bblk, Dsl, /*have_quat=*/true);
  MI_HIP(hipGetLastError());
  MI_TRY(partial_rows_to_slot(q, grid, 0, ctx->scalars + f_slot));
  const double *gn[1] = {q->grad_next->d};
  return dot_batch_to_slots(ctx, 1, gn, gn, 3 * q->N, g2_slot);
}

// ---- the lazily made resources: one ensure_* per group.  Each is idempotent and builds into locals, so a
// failure leaves q as it was. ----
// grad_next (3N): the gradient at the trial point of mi_so3n_trial / mi_so3n_armijo_trial; read by mi_so3n_model / _gradient
int ensure_grad_next(mi_so3n *q) { return q->grad_next ? MI_OK : vec_alloc(q->ctx, 3 * q->N, q->grad_next); }
// the trial arrays (the model's second set + Hess h + M^-1 grad): written by mi_so3n_trial, swapped in by mi_so3n_model
int ensure_trial_arrays(mi_so3n *q) {
  if (q->Dinv_next) return MI_OK;
  Owned<mi_vec> Dinv, Hh, Pg;
  DevPtr<double> Bblk, Dsl;
  MI_TRY(vec_alloc(q->ctx, 9 * q->N, Dinv));
  MI_TRY(vec_alloc(q->ctx, 3 * q->N, Hh));
  MI_TRY(vec_alloc(q->ctx, 3 * q->N, Pg));
  MI_TRY(dev_alloc(Bblk, q->padded * 9));
  MI_TRY(dev_alloc(Dsl, q->nslices * 9 * 64));
  q->Dinv_next = std::move(Dinv), q->Hh = std::move(Hh), q->Pg = std::move(Pg);
  q->Bblk_next = std::move(Bblk), q->Dsl_next = std::move(Dsl);
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_so3n_create(mi_ctx *ctx, size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt,
                   const double *w, mi_so3n **out) {
  MI_REQUIRE(ctx && out && (E == 0 || (ei && ej && Rt && w)), "null argument");
  So3Pack P;
  std::string err;
  MI_REQUIRE(so3_pack(N, E, ei, ej, Rt, w, ctx->cfg.so3_no_quat, ctx->cfg.so3_sort_nbr != 0, P, err) == 0, "%s", err.c_str());
  auto q = std::make_unique<mi_so3n>();
  q->ctx = ctx;
  q->N = N, q->E = E, q->nslices = P.nslices, q->nnzb = P.nnzb, q->padded = P.padded;
  q->sinc_quat = P.sinc_quat, q->w_nonneg = P.w_nonneg;
  MI_TRY(dev_upload(q->slice_ptr, P.slice_ptr.data(), P.slice_ptr.size()));
  MI_TRY(dev_upload(q->perm, P.perm.data(), P.perm.size()));
  MI_TRY(dev_alloc(q->Dsl, P.nslices * 9 * 64));
  if (!ctx->cfg.so3_no_rquat) MI_TRY(dev_alloc(q->Rq, N * 4));
  MI_TRY(dev_upload(q->nbr, P.nbr.data(), P.padded));
  MI_TRY(dev_alloc(q->Bblk, P.padded * 9));
  MI_TRY(dev_upload(q->Sinc, P.sinc.data(), P.sinc.size()));
  MI_TRY(dev_upload(q->winc, P.winc.data(), P.winc.size()));
  MI_TRY(vec_alloc(ctx, 9 * N, q->Dinv));
  // what the least-squares view and the reweighting upload on first use
  q->h_ij = std::move(P.h_ij), q->h_Se = std::move(P.h_Se), q->h_w = std::move(P.h_w), q->h_slot = std::move(P.h_slot);
  q->hess = borrowed_op(ctx, 3 * N, 0, so3_apply, nullptr, q.get());
  q->hess.apply_dots = so3_apply_dots;
  q->bj.ctx = ctx, q->bj.n = 3 * N, q->bj.impl = q.get(), q->bj.borrowed = true;
  q->bj.kind = 2, q->bj.data = q->Dinv->d, q->bj.apply = so3_bj_apply;  // fusable 3x3 block-Jacobi: data = inverse blocks
  *out = q.release();
  return MI_OK;
}

int mi_so3n_destroy(mi_so3n *q) {
  if (!q) return MI_OK;
  (void)hipStreamSynchronize(q->ctx->stream);
  delete q;
  return MI_OK;
}

// Read-only: which forms this problem took.  out = {measurements as unit quaternions (sinc_quat), neighbours gathered as
// quaternions (Rq), slices, incidences, padded incidence slots, workgroups of the model assembly (fewer than
// ceil(slices / 4): the grid-stride walk)}.  No GPU work (tests/test_gpu_so3n_edges.py).
int mi_debug_so3n_info(const mi_so3n *q, size_t out[6]) {
  MI_REQUIRE(q && out, "null argument");
  out[0] = q->sinc_quat ? 1 : 0;
  out[1] = q->Rq ? 1 : 0;
  out[2] = q->nslices;
  out[3] = q->nnzb;
  out[4] = q->padded;
  out[5] = (size_t)model_grid(q);
  return MI_OK;
}

int mi_so3n_objective(mi_so3n *q, const mi_vec *R, double *f) {
  MI_REQUIRE(q && R && f, "null argument");
  MI_REQUIRE(R->ctx == q->ctx && R->n == 9 * q->N, "R must hold N row-major 3x3 blocks");
  mi_ctx *ctx = q->ctx;
  // the incidence form of the sum (r05): the loop of the model assembly without its outputs -- what mi_so3n_trial gets
  // from the assembly at the trial point itself, bit for bit
  const int grid = model_grid(q);
  launch_assembly(q, SO3_OBJECTIVE, grid, R->d, nullptr, nullptr, nullptr, nullptr);
  MI_HIP(hipGetLastError());
  MI_TRY(partial_rows_to_slot(q, grid, 0, ctx->scalars + SLOT_MISC));
  double s = 0;
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, 1, &s));
  *f = .25 * s;  // (every edge from both ends)
  return MI_OK;
}

int mi_so3n_model(mi_so3n *q, const mi_vec *R, mi_vec *grad, mi_op **hess, mi_precon **block_jacobi) {
  MI_REQUIRE(q && R && grad, "null argument");
  MI_REQUIRE(R->ctx == q->ctx && R->n == 9 * q->N, "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(grad->n == 3 * q->N, "gradient must hold 3N doubles");
  touch(grad);
  if (q->trial.is(R)) {
    // R is the point mi_so3n_trial just evaluated: its model exists already
    // (the point of an Armijo trial is NOT one: only its gradient exists -- the full assembly below)
    std::swap(q->Dinv, q->Dinv_next);
    std::swap(q->Bblk, q->Bblk_next);
    std::swap(q->Dsl, q->Dsl_next);
    q->bj.data = q->Dinv->d;
    MI_TRY(mi_vec_copy(grad, q->grad_next.get()));
  } else {
    launch_assembly(q, SO3_MODEL, model_grid(q), R->d, grad->d, q->Dinv->d, q->Bblk.get(), q->Dsl.get());
    MI_HIP(hipGetLastError());
  }
  invalidate_models(q, false);
  q->R = R;
  q->R_serial = R->serial;
  if (hess) *hess = &q->hess;
  if (block_jacobi) *block_jacobi = &q->bj;
  return MI_OK;
}

int mi_so3n_retract(mi_so3n *q, const mi_vec *R, const mi_vec *xi, mi_vec *Y) {
  MI_REQUIRE(q && R && xi && Y, "null argument");
  MI_REQUIRE(R->n == 9 * q->N && Y->n == 9 * q->N && xi->n == 3 * q->N, "dimension mismatch");
  touch(Y);
  hipLaunchKernelGGL(k_so3_retract<false>, dim3(grid_for(q->ctx, q->N, 1)), dim3(kBlock), 0, q->ctx->stream, q->N,
                     (const double *)R->d, (const double *)xi->d, Y->d, (double *)nullptr);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// One trial step of a trust-region method at the point R the model is bound to (reference Riemannian/TNT.h:493-512,
// 573-585): Hess h with |h|^2, <g,h>, <h,Hess h>; R+ = retract(R, h); f(R+); and -- speculatively -- the model at R+
// (gradient, Hessian blocks, block-Jacobi inverse blocks) with |grad f(R+)|^2 and, if asked, |M+^-1 grad f(R+)|^2: ONE
// launch chain, ONE read-back.  Every number comes from the kernels, grids and summation orders the separate calls
// (mi_op_apply + mi_vec_dot_batch, mi_so3n_retract, mi_so3n_objective, mi_so3n_model, mi_vec_dot, mi_precon_apply)
// use.  out[6] = {f(R+), <h,h>, <g,h>, <h,Hess h>, |grad f(R+)|^2, |M+^-1 grad f(R+)|^2 (-1 unless with_precon)}.
int mi_so3n_trial(mi_so3n *q, const mi_vec *R, const mi_vec *h, const mi_vec *g, int with_precon, mi_vec *R_trial,
                  double out[6]) {
  MI_REQUIRE(q && R && h && g && R_trial && out, "null argument");
  MI_REQUIRE(bound_to(q->R, q->R_serial, R),
             "mi_so3n_trial: the model is not bound to this R (call mi_so3n_model first)");
  MI_REQUIRE(R->n == 9 * q->N && R_trial->n == 9 * q->N && h->n == 3 * q->N && g->n == 3 * q->N, "dimension mismatch");
  MI_REQUIRE(R_trial->d != R->d, "the trial point must not alias the current one");
  mi_ctx *ctx = q->ctx;
  ctx->fusion.fused_trial_steps++;
  const size_t N3 = 3 * q->N;
  MI_TRY(ensure_grad_next(q));
  MI_TRY(ensure_trial_arrays(q));
  invalidate_models(q, false);  // (grad_next is about to be overwritten)
  // (a) Hess h, then |h|^2, <g,h>, <h, Hess h> in one pass (as MI355::dot_batch does)
  MI_TRY(so3_apply(&q->hess, h, q->Hh.get()));
  {
    const double *xs[3] = {h->d, g->d, h->d}, *ys[3] = {h->d, h->d, q->Hh->d};
    MI_TRY(dot_batch_to_slots(ctx, 3, xs, ys, N3, SLOT_MISC));
  }
  // (b) R+ = R exp(hat h)
  MI_TRY(retract_trial(q, R, h, R_trial));
  // (c) + (d) the model at R+ into the second set of arrays, with f(R+) from the same pass (r05: the objective was an
  // edge pass of its own, 61 us and 416 MB at the fabric), and |grad f(R+)|^2
  MI_TRY(trial_tail(q, SO3_MODEL, R_trial, q->Dinv_next->d, q->Bblk_next.get(), q->Dsl_next.get(), SLOT_MISC + 3, SLOT_MISC + 4));
  if (with_precon) {
    MI_TRY(block3_apply(ctx, q->Dinv_next.get(), q->grad_next.get(), q->Pg.get()));
    const double *xs[1] = {q->Pg->d}, *ys[1] = {q->Pg->d};
    MI_TRY(dot_batch_to_slots(ctx, 1, xs, ys, N3, SLOT_MISC + 5));
  }
  // (e) one read-back
  static_assert(SLOT_MISC + 6 <= SLOT_GDIR, "slot map");
  double buf[6];
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, with_precon ? 6 : 5, buf));
  out[0] = .25 * buf[3];
  out[1] = buf[0];
  out[2] = buf[1];
  out[3] = buf[2];
  out[4] = buf[4];
  out[5] = with_precon ? buf[5] : -1.0;
  q->trial.set(R_trial);
  return MI_OK;
}

// Without a device the answer is MI_ERR_NO_DEVICE whatever the arguments (no context can exist); with one, a null
// argument is the usual MI_ERR_INVALID_ARGUMENT.
#define SO3_REQUIRE_ARGS(COND)                 \
  do {                                         \
    if (!(COND)) {                             \
      MI_TRY(ensure_device());                 \
      MI_REQUIRE(false, "null argument");      \
    }                                          \
  } while (0)

int mi_so3n_gradient(mi_so3n *q, const mi_vec *R, mi_vec *grad) {
  SO3_REQUIRE_ARGS(q && R && grad);
  MI_REQUIRE(R->ctx == q->ctx && R->n == 9 * q->N, "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(grad->ctx == q->ctx && grad->n == 3 * q->N, "gradient must hold 3N doubles");
  if (q->armijo.is(R) || q->trial.is(R)) {
    // the last Armijo trial (or, speculatively, the last trust-region trial) evaluated this very point: its gradient is
    // there.  Neither key is consumed: a following mi_so3n_model(R) still finds the speculative model of a TNT trial.
    return mi_vec_copy(grad, q->grad_next.get());
  }
  touch(grad);
  launch_assembly(q, SO3_GRAD, model_grid(q), R->d, grad->d, nullptr, nullptr, nullptr);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int mi_so3n_armijo_trial(mi_so3n *q, const mi_vec *R, const mi_vec *g, double t, mi_vec *h_out, mi_vec *R_trial,
                         double out[2]) {
  SO3_REQUIRE_ARGS(q && R && g && h_out && R_trial && out);
  MI_REQUIRE(R->ctx == q->ctx && g->ctx == q->ctx && h_out->ctx == q->ctx && R_trial->ctx == q->ctx,
             "vector belongs to another context");
  MI_REQUIRE(R->n == 9 * q->N && R_trial->n == 9 * q->N && g->n == 3 * q->N && h_out->n == 3 * q->N, "dimension mismatch");
  MI_REQUIRE(R_trial->d != R->d, "the trial point must not alias the current one");
  MI_REQUIRE(h_out->d != g->d, "the step must not alias the gradient");
  mi_ctx *ctx = q->ctx;
  ctx->fusion.fused_trial_steps++;
  MI_TRY(ensure_grad_next(q));  // (none of the Hessian-sized trial arrays)
  invalidate_models(q, false);  // (grad_next is about to be overwritten: the speculative model loses its gradient)
  // (a) h = -t g: the kernel of DeviceVector's `-t * g` (mi_vec_scale_to), then R+ = R exp(hat h)
  MI_TRY(mi_vec_scale_to(h_out, -t, g));
  MI_TRY(retract_trial(q, R, h_out, R_trial));
  // (b) + (c) grad f(R+) with f(R+) from the same pass, and |grad f(R+)|^2
  MI_TRY(trial_tail(q, SO3_GRAD, R_trial, nullptr, nullptr, nullptr, SLOT_MISC, SLOT_MISC + 1));
  // (d) one read-back
  double buf[2];
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, 2, buf));
  out[0] = .25 * buf[0];  // (every edge from both ends)
  out[1] = buf[1];
  q->armijo.set(R_trial);
  return MI_OK;
}

}  // extern "C"

namespace {

int edge_grid(const mi_so3n *q) {
  return (int)std::min<size_t>(std::max<size_t>(1, (q->E + kNlsBlock - 1) / kNlsBlock), (size_t)kMaxRows);
}
int node_grid(const mi_so3n *q) { return (int)std::min<size_t>(std::max<size_t>(1, (q->nslices + 3) / 4), (size_t)kMaxRows); }
EdgeView edge_view(const mi_so3n *q) { return EdgeView{q->E, q->e_ij.get(), q->Se.get(), q->swe.get()}; }
// winc, and gn_diag (may be null), from the per-edge weights w_cur
int launch_inc_reweight(mi_so3n *q, double *gn_diag) {
  mi_ctx *ctx = q->ctx;
  KScope ks(ctx, MI_K_SO3_INC_REWEIGHT);
  hipLaunchKernelGGL(k_so3_inc_reweight, dim3(node_grid(q)), dim3(kNlsBlock), 0, ctx->stream, view(q),
                     (const uint32_t *)q->slot_edge.get(), (const double *)q->w_cur.get(), q->winc.get(), gn_diag);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
// the edge streams e_ij, Se (static): read by k_so3_residual, k_so3_jac, k_so3_edge_weight
int ensure_edge_streams(mi_so3n *q) {
  if (q->e_ij) return MI_OK;
  DevPtr<double> Se; DevPtr<int2> ij;
  MI_TRY(dev_upload(Se, q->h_Se.data(), q->h_Se.size()));
  MI_TRY(dev_upload(ij, (const int2 *)q->h_ij.data(), q->E));
  q->Se = std::move(Se), q->e_ij = std::move(ij);
  return MI_OK;
}
// the slot words slot_edge (static): read by k_so3_jact, k_so3_inc_reweight
int ensure_slot_words(mi_so3n *q) {
  if (q->slot_edge) return MI_OK;
  MI_REQUIRE(q->E < ((size_t)1 << 31), "the incidence -> edge words hold edge numbers below 2^31");
  return dev_upload(q->slot_edge, q->h_slot.data(), q->h_slot.size());
}
// The weights in force are w_cur on the device once a reweighting has made it, else h_w on the host: ensure_swe and
// ensure_gn_scaling are the two places that decide between them (a reweighting rewrites what exists of both itself).
// swe = sqrt(w_e): read by k_so3_residual, k_so3_jac; rewritten by k_so3_edge_weight
int ensure_swe(mi_so3n *q) {
  if (q->swe) return MI_OK;
  DevPtr<double> swe;
  if (q->w_cur) {
    MI_TRY(dev_alloc(swe, q->E));
    hipLaunchKernelGGL(k_so3_sqrt_w, dim3(edge_grid(q)), dim3(kNlsBlock), 0, q->ctx->stream, q->E, (const double *)q->w_cur.get(),
                       swe.get());
    MI_HIP(hipGetLastError());
  } else {
    std::vector<double> sw(q->E);
    for (size_t e = 0; e < q->E; ++e) sw[e] = std::sqrt(q->h_w[e]);
    MI_TRY(dev_upload(swe, sw.data(), sw.size()));
  }
  q->swe = std::move(swe);
  return MI_OK;
}
// gn_diag = 1 / sqrt(2 degw_i) and the diagonal operator on it (mi_so3n_gn_scaling); rewritten by k_so3_inc_reweight
int ensure_gn_scaling(mi_so3n *q) {
  if (q->gn_op) return MI_OK;
  Owned<mi_vec> diag;
  MI_TRY(vec_alloc(q->ctx, 3 * q->N, diag));
  if (q->w_cur) {
    // by the pass that keeps it current (winc is rewritten to itself)
    touch(diag.get());
    MI_TRY(launch_inc_reweight(q, diag->d));
  } else {
    std::vector<double> degw(q->N, 0.0), d(3 * q->N);
    for (size_t e = 0; e < q->E; ++e) {
      degw[(size_t)q->h_ij[2 * e]] += q->h_w[e];
      degw[(size_t)q->h_ij[2 * e + 1]] += q->h_w[e];
    }
    for (size_t i = 0; i < q->N; ++i) d[3 * i] = d[3 * i + 1] = d[3 * i + 2] = degw[i] > 0 ? 1.0 / std::sqrt(2 * degw[i]) : 1.0;
    MI_TRY(mi_vec_upload(diag.get(), d.data(), d.size()));
  }
  mi_op *op = nullptr;
  MI_TRY(mi_op_create_diag(q->ctx, diag.get(), &op));
  op->borrowed = true;
  q->gn_diag = std::move(diag);
  q->gn_op.reset(op);
  return MI_OK;
}
// Jrot (9N): written by mi_so3n_jacobian, read by k_so3_jac, k_so3_jact
int ensure_jrot(mi_so3n *q) { return q->Jrot ? MI_OK : dev_alloc(q->Jrot, q->N * 9); }
// w0 (the creation-time weights) and w_cur (written by k_so3_edge_weight): mi_so3n_reweight
int ensure_weights(mi_so3n *q) {
  if (q->w_cur) return MI_OK;
  DevPtr<double> w0, w_cur;
  MI_TRY(dev_upload(w0, q->h_w.data(), q->E));
  MI_TRY(dev_alloc(w_cur, q->E));
  q->w0 = std::move(w0), q->w_cur = std::move(w_cur);
  return MI_OK;
}
// what mi_so3n_residual (and, with_jacobian, mi_so3n_jacobian) reads
int ensure_nls(mi_so3n *q, bool with_jacobian) {
  MI_REQUIRE(q->w_nonneg, "the least-squares form F_e = sqrt(w_e) (R_j - R_i Rt_e) needs weights >= 0");
  MI_REQUIRE(!q->ctx->uniform_grid, "the least-squares view of mi_so3n is single-context");
  MI_TRY(ensure_edge_streams(q));
  MI_TRY(ensure_swe(q));
  if (with_jacobian) MI_TRY(ensure_slot_words(q));
  if (with_jacobian) MI_TRY(ensure_jrot(q));
  return MI_OK;
}

int so3_jac_launch(mi_op *self, const mi_vec *in, mi_vec *out, const double *scale, const int *mode, const int *gate,
                   double *partials, int *nparts) {
  mi_so3n *q = (mi_so3n *)self->impl;
  mi_ctx *ctx = q->ctx;
  const int grid = edge_grid(q);
  const bool fused = scale != nullptr;
  KScope ks(ctx, MI_K_SO3_JAC);
  DISPATCH_FLAG(fused, FUSED, DISPATCH_FLAG(q->sinc_quat, SQ, DISPATCH_FLAG(q->jac_quat, GQ,
      hipLaunchKernelGGL((k_so3_jac<FUSED, SQ, GQ>), dim3(grid), dim3(kNlsBlock), 0, ctx->stream, edge_view(q),
                         (const double *)q->Jrot.get(), (const double *)in->d, out->d, scale, mode, gate, partials))));
  if (nparts) *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}
int so3_jact_launch(mi_op *self, const mi_vec *in, mi_vec *out, const double *scale, const int *mode, const int *gate,
                    double *partials, int *nparts) {
  mi_so3n *q = (mi_so3n *)self->impl;
  mi_ctx *ctx = q->ctx;
  const int grid = node_grid(q);
  const bool fused = scale != nullptr;
  KScope ks(ctx, MI_K_SO3_JACT);
  DISPATCH_FLAG(fused, FUSED, DISPATCH_FLAG(q->sinc_quat, SQ, DISPATCH_FLAG(q->jac_quat, GQ,
      hipLaunchKernelGGL((k_so3_jact<FUSED, SQ, GQ>), dim3(grid), dim3(kNlsBlock), 0, ctx->stream, view(q),
                         (const double *)q->Jrot.get(), (const double *)q->Sinc.get(), (const double *)q->winc.get(),
                         (const uint32_t *)q->slot_edge.get(), (const double *)in->d, out->d, scale, mode, gate, partials))));
  if (nparts) *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}
int so3_jac_apply(mi_op *self, const mi_vec *in, mi_vec *out) {
  return so3_jac_launch(self, in, out, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int so3_jact_apply(mi_op *self, const mi_vec *in, mi_vec *out) {
  return so3_jact_launch(self, in, out, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int so3_jac_sub_scaled(mi_op *self, const mi_vec *in, const double *scale, const int *mode, const int *gate, mi_vec *inout,
                       double *partials, int *nparts) {
  MI_REQUIRE(scale && mode && partials && nparts, "null argument");
  return so3_jac_launch(self, in, inout, scale, mode, gate, partials, nparts);
}
int so3_jact_sub_scaled(mi_op *self, const mi_vec *in, const double *scale, const int *mode, const int *gate, mi_vec *inout,
                        double *partials, int *nparts) {
  MI_REQUIRE(scale && mode && partials && nparts, "null argument");
  return so3_jact_launch(self, in, inout, scale, mode, gate, partials, nparts);
}

}  // namespace

extern "C" {

int mi_so3n_residual(mi_so3n *q, const mi_vec *R, mi_vec *F, double *sqnorm) {
  SO3_REQUIRE_ARGS(q && R && F);
  MI_REQUIRE(R->ctx == q->ctx && R->n == 9 * q->N, "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(F->ctx == q->ctx && F->n == 9 * q->E, "the residual must hold 9 doubles per edge");
  mi_ctx *ctx = q->ctx;
  if (q->E == 0) {
    if (sqnorm) *sqnorm = 0;
    return MI_OK;
  }
  MI_TRY(ensure_nls(q, false));
  touch(F);
  // quaternion gathers only at a point whose records the retraction of a fused trial step left in Rq; any other point
  // is read as it is given (72-byte rows): Rq is not written here, nor anything else a bound Jacobian reads
  const bool gq = q->Rq && q->rq.is(R);
  const int grid = edge_grid(q);
  {
    KScope ks(ctx, MI_K_SO3_RESIDUAL);
    DISPATCH_FLAG(q->sinc_quat, SQ, DISPATCH_FLAG(gq, GQ,
        hipLaunchKernelGGL((k_so3_residual<SQ, GQ>), dim3(grid), dim3(kNlsBlock), 0, ctx->stream, edge_view(q),
                           GQ ? (const double *)q->Rq.get() : (const double *)R->d, F->d, ctx->partials2)));
  }
  MI_HIP(hipGetLastError());
  if (sqnorm) {
    MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, grid, 1, ctx->scalars + SLOT_MISC));
    MI_TRY(read_slots_sync(ctx, SLOT_MISC, 1, sqnorm));
  }
  return MI_OK;
}

int mi_so3n_jacobian(mi_so3n *q, const mi_vec *R, mi_op **dF, mi_op **dFt) {
  SO3_REQUIRE_ARGS(q && R && dF && dFt);
  MI_REQUIRE(R->ctx == q->ctx && R->n == 9 * q->N, "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(q->E > 0, "mi_so3n_jacobian: the problem has no edges (a 3N -> 0 operator)");
  mi_ctx *ctx = q->ctx;
  MI_TRY(ensure_nls(q, true));
  // the linearisation's own copy of the rotations: TNLS evaluates F at trial points while LSQR still uses these operators
  q->jac_quat = q->Rq && q->rq.is(R);
  const size_t words = q->jac_quat ? 4 : 9;
  MI_HIP(hipMemcpyAsync(q->Jrot.get(), q->jac_quat ? q->Rq.get() : R->d, q->N * words * sizeof(double), hipMemcpyDeviceToDevice,
                        ctx->stream));
  q->dF = borrowed_op(ctx, 3 * q->N, 9 * q->E, so3_jac_apply, so3_jac_sub_scaled, q);
  q->dFt = borrowed_op(ctx, 9 * q->E, 3 * q->N, so3_jact_apply, so3_jact_sub_scaled, q);
  *dF = &q->dF;
  *dFt = &q->dFt;
  return MI_OK;
}

int mi_so3n_gn_scaling(mi_so3n *q, mi_op **M) {
  SO3_REQUIRE_ARGS(q && M);
  MI_REQUIRE(q->w_nonneg, "the Gauss-Newton scaling 1 / sqrt(2 degw) needs weights >= 0");
  MI_TRY(ensure_gn_scaling(q));
  *M = q->gn_op.get();
  return MI_OK;
}

// ---- robust loss by edge reweighting (kernels: k_so3_edge_weight, k_so3_inc_reweight) ----
int mi_so3n_reweight(mi_so3n *q, const mi_vec *R, int kind, double c, double info[3]) {
  SO3_REQUIRE_ARGS(q);
  mi_ctx *ctx = q->ctx;
  MI_REQUIRE(kind >= SO3_ROBUST_L2 && kind <= SO3_ROBUST_GM, "unknown robust kernel %d", kind);
  MI_REQUIRE(kind == SO3_ROBUST_L2 || (std::isfinite(c) && c > 0), "the robust scale c must be finite and > 0");
  MI_REQUIRE(R || kind == SO3_ROBUST_L2, "R may be null only for MI_ROBUST_L2");
  MI_REQUIRE(!R || (R->ctx == q->ctx && R->n == 9 * q->N), "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(!ctx->uniform_grid, "the reweighting of mi_so3n is single-context");
  if (kind == SO3_ROBUST_L2) c = 1.0;
  invalidate_models(q, true);  // (what was worked out with the old weights)
  if (q->E == 0) {
    if (info) info[0] = info[1] = info[2] = 0.0;
    return MI_OK;
  }
  // first use: the one-time uploads (sync)
  MI_TRY(ensure_edge_streams(q));
  MI_TRY(ensure_slot_words(q));
  MI_TRY(ensure_weights(q));
  const int grid = edge_grid(q);
  {
    KScope ks(ctx, MI_K_SO3_EDGE_WEIGHT);
    DISPATCH_FLAG(q->sinc_quat, SQ,
        hipLaunchKernelGGL((k_so3_edge_weight<SQ>), dim3(grid), dim3(kNlsBlock), 0, ctx->stream, edge_view(q),
                           (const double *)q->w0.get(), R ? (const double *)R->d : (const double *)nullptr, kind, c,
                           q->w_cur.get(), q->swe.get(), ctx->partials2));
  }
  MI_HIP(hipGetLastError());
  touch(q->gn_diag.get());
  MI_TRY(launch_inc_reweight(q, q->gn_diag ? q->gn_diag->d : nullptr));
  if (info) {
    MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, grid, 3, ctx->scalars + SLOT_MISC));
    MI_TRY(read_slots_sync(ctx, SLOT_MISC, 3, info));  // the one read-back
  }
  return MI_OK;
}

int mi_so3n_weights(mi_so3n *q, double *w_host) {
  SO3_REQUIRE_ARGS(q && (w_host || q->E == 0));
  if (q->E == 0) return MI_OK;
  if (!q->w_cur) {
    std::memcpy(w_host, q->h_w.data(), q->E * sizeof(double));
    return MI_OK;
  }
  MI_TRY(stream_wait(q->ctx, "mi_so3n_weights"));
  MI_HIP(hipMemcpy(w_host, q->w_cur.get(), q->E * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OK;
}

// ---- global-optimality certificate (kernels: k_so3_cert_diag, k_so3_cert_panel) ----
}  // extern "C"

namespace {

// q->cert / q->lap: Esl, written by k_so3_cert_diag / k_so3_lap_diag, read by k_so3_cert_panel (k_so3_lap_jacobi); Y
int ensure_cert_slot(mi_so3n *q, Owned<mi_so3n_cert> &slot, bool with_Y) {
  if (slot) return MI_OK;
  Owned<mi_so3n_cert> c(new mi_so3n_cert());
  c->q = q;
  MI_TRY(dev_alloc(c->Esl, q->nslices * 6 * 64));
  if (with_Y) MI_TRY(vec_alloc(q->ctx, 9 * q->N, c->Y));
  slot = std::move(c);
  return MI_OK;
}
int cert_launch(const mi_so3n_cert *c, const CertCols &X, int k, double *Z) {
  const mi_so3n *q = c->q;
  mi_ctx *ctx = q->ctx;
  const int KCsel = k == 1 ? 1 : k <= 4 ? 4 : 8;
  const dim3 grid((unsigned)std::min<size_t>(std::max<size_t>(1, (q->nslices + 3) / 4), 4096), (unsigned)((k + KCsel - 1) / KCsel));
#define CERT_PANEL(KCV)                                                                                                     \
  DISPATCH_FLAG(q->sinc_quat, SQ,                                                                                           \
                hipLaunchKernelGGL((k_so3_cert_panel<KCV, SQ>), grid, dim3(256), 0, ctx->stream, view(q),                   \
                                   (const double *)q->Sinc.get(), (const double *)q->winc.get(), (const double *)c->Esl.get(), X, k, Z))
  if (KCsel == 1) { CERT_PANEL(1); }
  else if (KCsel == 4) { CERT_PANEL(4); }
  else { CERT_PANEL(8); }
#undef CERT_PANEL
  MI_HIP(hipGetLastError());
  return MI_OK;
}
constexpr int kCertMaxK = 96;  // the widest panel of the LOBPCG building blocks (lobpcg.hip: kGramMaxK)
// Z (3N x k) against an input block of `cols` columns: both in the problem's context, large enough, not overlapping
// (same_ok: or one and the same panel)
int cert_check_io(const mi_so3n *q, const mi_vec *X, int cols, const mi_vec *Z, int k, bool same_ok = false) {
  const size_t m = 3 * q->N;
  MI_REQUIRE(X->ctx == q->ctx && Z->ctx == q->ctx, "panel belongs to another context");
  MI_REQUIRE(X->n >= m * (size_t)cols, "X holds %zu doubles, needs 3N * k = %zu * %d", X->n, m, cols);
  MI_REQUIRE(Z->n >= m * (size_t)k, "Z holds %zu doubles, needs 3N * k = %zu * %d", Z->n, m, k);
  const bool apart = Z->d + m * (size_t)k <= X->d || X->d + m * (size_t)cols <= Z->d;
  if (same_ok) MI_REQUIRE(Z->d == X->d || apart, "input and output panels must be the same or not overlap");
  else MI_REQUIRE(apart, "input and output panels must not overlap");
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_so3n_certificate(mi_so3n *q, const mi_vec *R, mi_so3n_cert **out, double info[3]) {
  SO3_REQUIRE_ARGS(q && R && out && info);
  MI_REQUIRE(R->ctx == q->ctx && R->n == 9 * q->N, "R must hold N row-major 3x3 blocks");
  mi_ctx *ctx = q->ctx;
  MI_REQUIRE(!ctx->uniform_grid, "the certificate of mi_so3n is single-context");
  MI_TRY(ensure_cert_slot(q, q->cert, true));
  mi_so3n_cert *c = q->cert.get();
  touch(c->Y.get());
  // the neighbours gathered as mi_so3n_objective gathers them (quaternion records when the problem keeps them: those the
  // retraction of a fused trial step left for this very point, else converted here first)
  const bool gq = q->Rq != nullptr;
  ensure_rq(q, R->d, q->rq.is(R));
  const int grid = model_grid(q);
  DISPATCH_FLAG(q->sinc_quat, SQ, DISPATCH_FLAG(gq, GQ,
      hipLaunchKernelGGL((k_so3_cert_diag<SQ, GQ>), dim3(grid), dim3(256), 0, ctx->stream, view(q), (const double *)R->d,
                         (const double *)q->Rq.get(), (const double *)q->Sinc.get(), (const double *)q->winc.get(), c->Esl.get(),
                         c->Y->d, ctx->partials2)));
  MI_HIP(hipGetLastError());
  for (int which = 0; which < 3; ++which) MI_TRY(partial_rows_to_slot(q, grid, which, ctx->scalars + SLOT_MISC + which));
  double buf[3];
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, 3, buf));  // the one read-back
  info[0] = .25 * buf[0];  // (every edge from both ends)
  info[1] = .5 * std::sqrt(buf[1]);  // |skew Q|_F with skew Q_i = (Q_i - Q_i') / 2: the sum holds |Q_i - Q_i'|_F^2
  info[2] = buf[2];
  *out = c;
  return MI_OK;
}

int mi_so3n_cert_apply(mi_so3n_cert *c, int k, const mi_vec *X, mi_vec *Z) {
  SO3_REQUIRE_ARGS(c && X && Z);
  MI_REQUIRE(k >= 1 && k <= kCertMaxK, "panel width must be in [1,%d]", kCertMaxK);
  MI_TRY(cert_check_io(c->q, X, k, Z, k));
  touch(Z);
  return cert_launch(c, CertCols{{X->d, X->d, X->d}, k, k}, k, Z->d);
}

int mi_so3n_cert_apply_blocks(mi_so3n_cert *c, const mi_panel_blocks *X, mi_vec *Z) {
  SO3_REQUIRE_ARGS(c && X && Z);
  MI_REQUIRE(X->nblocks >= 1 && X->nblocks <= 3, "a panel has 1 to 3 column blocks");
  int k = 0;
  for (int b = 0; b < X->nblocks; ++b) {
    MI_REQUIRE(X->block[b] && X->cols[b] >= 1, "column block %d is empty", b);
    k += X->cols[b];
  }
  MI_REQUIRE(k <= kCertMaxK, "panel width must be in [1,%d]", kCertMaxK);
  for (int b = 0; b < X->nblocks; ++b) MI_TRY(cert_check_io(c->q, X->block[b], X->cols[b], Z, k));
  const double *b0 = X->block[0]->d, *b1 = X->nblocks > 1 ? X->block[1]->d : b0, *b2 = X->nblocks > 2 ? X->block[2]->d : b1;
  const int n0 = X->nblocks > 1 ? X->cols[0] : k, n01 = X->nblocks > 2 ? n0 + X->cols[1] : k;
  touch(Z);
  return cert_launch(c, CertCols{{b0, b1, b2}, n0, n01}, k, Z->d);
}

int mi_so3n_cert_null_panel(mi_so3n_cert *c, mi_vec **Y) {
  SO3_REQUIRE_ARGS(c && Y);
  MI_REQUIRE(c->Y, "the connection Laplacian of mi_so3n_laplacian has no panel Y");
  *Y = c->Y.get();
  return MI_OK;
}

}  // extern "C"

// ---- spectral initialisation (kernels: k_so3_lap_diag, k_so3_lap_jacobi, k_so3_round_sign, k_so3_round) ----
namespace {

// the Laplacian's handle, its diagonal written from the weights in force
int lap_refresh(mi_so3n *q) {
  mi_ctx *ctx = q->ctx;
  MI_REQUIRE(!ctx->uniform_grid, "the connection Laplacian of mi_so3n is single-context");
  MI_TRY(ensure_cert_slot(q, q->lap, false));
  hipLaunchKernelGGL(k_so3_lap_diag, dim3(node_grid(q)), dim3(256), 0, ctx->stream, view(q), (const double *)q->winc.get(),
                     q->lap->Esl.get());
  MI_HIP(hipGetLastError());
  return MI_OK;
}
// round_words (RW_WORDS): what k_so3_round_sign / k_so3_round count and mi_so3n_round / mi_so3n_project read back
int ensure_round_words(mi_so3n *q) { return q->round_words ? MI_OK : dev_alloc(q->round_words, RW_WORDS); }
// the count words of one rounding call, zeroed (RW_EXTREME: the neutral element of the call's min or max)
int round_words_init(mi_so3n *q, double extreme) {
  MI_TRY(ensure_round_words(q));
  unsigned long long bits;
  std::memcpy(&bits, &extreme, sizeof(bits));
  hipLaunchKernelGGL(k_so3_round_init, dim3(1), dim3(1), 0, q->ctx->stream, q->round_words.get(), bits);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
int round_words_read(mi_so3n *q, const char *what, unsigned long long words[RW_WORDS]) {
  MI_TRY(stream_wait(q->ctx, what));
  MI_HIP(hipMemcpy(words, q->round_words.get(), RW_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return MI_OK;
}
double word_as_double(unsigned long long w) {
  double d;
  std::memcpy(&d, &w, sizeof(d));
  return d;
}

}  // namespace

extern "C" {

int mi_so3n_laplacian(mi_so3n *q, mi_so3n_cert **out) {
  SO3_REQUIRE_ARGS(q && out);
  MI_TRY(lap_refresh(q));
  *out = q->lap.get();
  return MI_OK;
}

int mi_so3n_lap_jacobi(mi_so3n *q, int k, const mi_vec *X, mi_vec *Z) {
  SO3_REQUIRE_ARGS(q && X && Z);
  MI_REQUIRE(k >= 1 && k <= kCertMaxK, "panel width must be in [1,%d]", kCertMaxK);
  MI_TRY(cert_check_io(q, X, k, Z, k, /*same_ok=*/true));
  if (!q->lap) MI_TRY(lap_refresh(q));  // (else: the diagonal of the latest mi_so3n_laplacian call)
  touch(Z);
  hipLaunchKernelGGL(k_so3_lap_jacobi, dim3(node_grid(q)), dim3(256), 0, q->ctx->stream, view(q), (const double *)q->lap->Esl.get(),
                     k, (const double *)X->d, Z->d);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int mi_so3n_round(mi_so3n *q, const mi_vec *V, mi_vec *R, double info[4]) {
  SO3_REQUIRE_ARGS(q && V && R);
  const size_t n9 = 9 * q->N;
  MI_REQUIRE(V->ctx == q->ctx && V->n >= n9, "V must hold the column-major 3N x 3 panel");
  MI_REQUIRE(R->ctx == q->ctx && R->n == n9, "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(R->d + n9 <= V->d || V->d + n9 <= R->d, "the panel and the point must not overlap");
  mi_ctx *ctx = q->ctx;
  MI_TRY(round_words_init(q, HUGE_VAL));
  touch(R);
  const int grid = grid_for(ctx, q->N, 1);
  hipLaunchKernelGGL(k_so3_round_sign, dim3(grid), dim3(256), 0, ctx->stream, q->N, (const double *)V->d, q->round_words.get());
  hipLaunchKernelGGL(k_so3_round<true>, dim3(grid), dim3(256), 0, ctx->stream, q->N, (const double *)V->d, R->d,
                     q->round_words.get());
  MI_HIP(hipGetLastError());
  if (info) {
    unsigned long long w[RW_WORDS];
    MI_TRY(round_words_read(q, "mi_so3n_round", w));  // the one read-back
    info[0] = (double)w[RW_NEG];
    info[1] = (long long)w[RW_SIGN] < 0 ? 1.0 : 0.0;
    info[2] = (double)w[RW_DEGENERATE];
    info[3] = w[RW_DEGENERATE] == q->N ? std::nan("") : word_as_double(w[RW_EXTREME]);
  }
  return MI_OK;
}

int mi_so3n_project(mi_so3n *q, const mi_vec *M, mi_vec *R, double info[3]) {
  SO3_REQUIRE_ARGS(q && M && R);
  const size_t n9 = 9 * q->N;
  MI_REQUIRE(M->ctx == q->ctx && M->n == n9, "M must hold N row-major 3x3 blocks");
  MI_REQUIRE(R->ctx == q->ctx && R->n == n9, "R must hold N row-major 3x3 blocks");
  MI_REQUIRE(R->d == M->d || R->d + n9 <= M->d || M->d + n9 <= R->d, "R must be M itself or not overlap it");
  mi_ctx *ctx = q->ctx;
  MI_TRY(round_words_init(q, 0.0));
  touch(R);
  hipLaunchKernelGGL(k_so3_round<false>, dim3(grid_for(ctx, q->N, 1)), dim3(256), 0, ctx->stream, q->N, (const double *)M->d,
                     R->d, q->round_words.get());
  MI_HIP(hipGetLastError());
  if (info) {
    unsigned long long w[RW_WORDS];
    MI_TRY(round_words_read(q, "mi_so3n_project", w));  // the one read-back
    info[0] = word_as_double(w[RW_EXTREME]);
    info[1] = (double)w[RW_DEGENERATE];
    info[2] = (double)w[RW_NEG];
  }
  return MI_OK;
}

}  // extern "C"
