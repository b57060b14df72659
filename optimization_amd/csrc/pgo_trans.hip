// pgo_trans.hip -- the translation half of a pose graph on the device (second stage of chordal initialisation; the step
// SE-Sync performs after its rotation solve).  With the rotations R (9N, row-major blocks: the point of mi_so3n) fixed,
// the positions of the edges e = (i -> j) with relative translation tt_e and weight tau_e solve
//     min_t  f_tau(R, t) = 1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2    <=>    L_a t = b(R)   (gauge t_anchor = 0),
//     b_i = sum over the slots of node i:  -tau_e R_i tt_e   (i is the first node of e)
//                                          +tau_e R_k tt_e   (e = (k -> i))
// L_a (x) I_3 is the anchored tau-weighted graph Laplacian on the N x 3 row-major field t: SPD on the anchor's component,
// Jacobi-preconditioned, and exactly the p = 3 CSR product with the curvature dots inside that the fused STPCG solves.
// There is NO Laplacian kernel here on purpose: in incidence form it would stream 12 bytes per entry (tau + neighbour),
// which is what the CSR path streams, and the CSR path has the fused dots and the format choice already.
// What is here: the two passes that depend on R, and the object that ties them to mi_csr / mi_op / mi_precon / mi_stpcg.
//
// Layouts (pgo_trans_pack.h): the node-centric SELL-64-sigma incidence layout of so3_pack.h (slice_ptr, perm, nbr, one slot
// word edge << 1 | first) with tinc (3 components, component-major per slot) and tauinc (0 on padding and on every slot of
// the anchor's and the zero-degree nodes' rows); per-edge streams (i, j), tt (component-major), tau in the caller's order.
//
// k_pgo_trans_rhs: one lane per node in slice order (the walk of k_bsr3_spmv), the incidences summed in slot order, no
//   atomics: the same bits on every run.  A slot with tau = 0 contributes nothing and gathers nothing (b_anchor = 0 and
//   b = 0 on zero-degree nodes exactly, whatever R holds).
//   Algorithmic bytes: 40 per slot (24 tinc + 8 tauinc + 4 nbr + 4 word; streamed non-temporally)
//                      + 72 per second-node incidence (the neighbour's row of R: a random gather; E of them)
//                      + 100 N (4 perm + 72 own row of R + 24 written).
// k_pgo_trans_residual: one thread per edge in the caller's order: r_e = t_j - t_i - R_i tt_e, optionally written; the
//   workgroup partial rows of sum 1/2 tau_e |r_e|^2 (component 0) and of max_e |r_e|^2 (component 1) in ctx->partials2,
//   reduced in a fixed order.  Algorithmic bytes: 160 E (8 end points + 24 tt + 8 tau + 72 R_i + 48 t_i, t_j) [+ 24 E written].
// Both form R tt through rot_apply with contraction off: the same bits in the two passes.  Both are bound by the random
// 72-byte gathers (1.56 cache lines each on average), like the model assembly of so3.hip.
#include <algorithm>
#include <cmath>

#include "mi_internal.h"
#include "pgo_trans_pack.h"

using namespace mi;

namespace {

constexpr int kPgoEdgeBlock = 256;  // one thread per edge, <= kMaxRows workgroups (grid-stride beyond)
// mi_pgo_trans_solve runs mi_stpcg as plain PCG: a trust-region radius that never binds.  The boundary test compares
// |s|_M^2 with Delta^2 = 1e300 (finite): an iterate would need |t|_M >= 1e150 to reach it.
constexpr double kPgoDelta = 1e150;

struct PgoIncView {
  size_t nslices;
  const long long *__restrict__ slice_ptr;
  const int *__restrict__ perm;       // node owned by (slice, lane), -1: padding lane
  const int *__restrict__ nbr;        // neighbour node (padding: own node)
  const uint32_t *__restrict__ slot;  // edge << 1 | (the slot's node is the first node of the edge)
  const double *__restrict__ tinc;    // component c of slot (k, lane) at (k * 3 + c) * 64 + lane
  const double *__restrict__ tauinc;
};
struct PgoEdgeView {
  size_t E;
  const int2 *__restrict__ ij;
  const double *__restrict__ tt;  // component c of edge e at c * E + e
  const double *__restrict__ tau;
};

// v = M x for a row-major 3 x 3 block, contraction off: the right-hand side and the residual pass get the same bits
__device__ __forceinline__ void rot_apply(const double *M, double x0, double x1, double x2, double *v) {
#pragma clang fp contract(off)
  v[0] = M[0] * x0 + M[1] * x1 + M[2] * x2;
  v[1] = M[3] * x0 + M[4] * x1 + M[5] * x2;
  v[2] = M[6] * x0 + M[7] * x1 + M[8] * x2;
}
__device__ __forceinline__ void load_row9(const double *__restrict__ R, size_t i, double *M) {
#pragma unroll
  for (int c = 0; c < 9; ++c) M[c] = R[9 * i + c];
}

__global__ __launch_bounds__(kBlock) void k_pgo_trans_rhs(PgoIncView inc, const double *__restrict__ R, double *__restrict__ b) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ngroups = (inc.nslices + kWaves - 1) / kWaves;
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t g0 = (ngroups * lb) / nb, g1 = (ngroups * (lb + 1)) / nb;
  for (size_t g = g0; g < g1; ++g) {
    const size_t slice = g * kWaves + w;
    if (slice >= inc.nslices) continue;
    const int node = inc.perm[slice * 64 + lane];
    if (node < 0) continue;
    const size_t i = (size_t)node;
    double Ri[9];
    load_row9(R, i, Ri);
    double b0 = 0, b1 = 0, b2 = 0;
    const long long k0 = inc.slice_ptr[slice], k1 = inc.slice_ptr[slice + 1];
    for (long long k = k0; k < k1; ++k) {
      const size_t e0 = (size_t)k * 64 + lane;
      const double tau = __builtin_nontemporal_load(inc.tauinc + e0);
      const int j = __builtin_nontemporal_load(inc.nbr + e0);
      const uint32_t word = __builtin_nontemporal_load(inc.slot + e0);
      const double *T = inc.tinc + (size_t)k * 3 * 64 + lane;
      const double x0 = __builtin_nontemporal_load(T), x1 = __builtin_nontemporal_load(T + 64),
                   x2 = __builtin_nontemporal_load(T + 128);
      if (tau == 0.0) continue;  // padding, a zero weight, the anchor's row, a zero-degree node's row
      double v[3];
      if (word & 1u) {
        rot_apply(Ri, x0, x1, x2, v);
        b0 -= tau * v[0]; b1 -= tau * v[1]; b2 -= tau * v[2];
      } else {
        double Rk[9];
        load_row9(R, (size_t)j, Rk);
        rot_apply(Rk, x0, x1, x2, v);
        b0 += tau * v[0]; b1 += tau * v[1]; b2 += tau * v[2];
      }
    }
    b[3 * i] = b0; b[3 * i + 1] = b1; b[3 * i + 2] = b2;
  }
}

template <bool WRITE>
__global__ __launch_bounds__(kPgoEdgeBlock) void k_pgo_trans_residual(PgoEdgeView ev, const double *__restrict__ R,
                                                                     const double *__restrict__ t, double *__restrict__ r_out,
                                                                     double *__restrict__ partials) {
#pragma clang fp contract(off)
  constexpr int NW = kPgoEdgeBlock / 64;
  __shared__ double lds[NW], mlds[NW];
  double acc[1] = {0};
  double rmax = 0;
  const size_t stride = (size_t)gridDim.x * kPgoEdgeBlock;
  for (size_t e = (size_t)blockIdx.x * kPgoEdgeBlock + threadIdx.x; e < ev.E; e += stride) {
    const int2 ij = ev.ij[e];
    const size_t i = (size_t)ij.x, j = (size_t)ij.y;
    double Ri[9], v[3];
    load_row9(R, i, Ri);
    rot_apply(Ri, ev.tt[e], ev.tt[ev.E + e], ev.tt[2 * ev.E + e], v);
    const double r0 = t[3 * j] - t[3 * i] - v[0], r1 = t[3 * j + 1] - t[3 * i + 1] - v[1],
                 r2 = t[3 * j + 2] - t[3 * i + 2] - v[2];
    if (WRITE) {
      r_out[3 * e] = r0; r_out[3 * e + 1] = r1; r_out[3 * e + 2] = r2;
    }
    const double rr = (r0 * r0 + r1 * r1) + r2 * r2;
    acc[0] += .5 * ev.tau[e] * rr;
    rmax = fmax(rmax, rr);
  }
  // max |r|^2 over the workgroup: order does not matter for a maximum, the shape is fixed all the same
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) rmax = fmax(rmax, __shfl_down(rmax, off, 64));
  if ((threadIdx.x & 63) == 0) mlds[threadIdx.x >> 6] = rmax;
  block_partials_store_nw<1, NW>(acc, lds, partials);  // (its barriers publish mlds as well)
  if (threadIdx.x == 0) {
    double m = mlds[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) m = fmax(m, mlds[q]);
    partials[(size_t)kMaxRows + blockIdx.x] = m;
  }
}
// slot[0] = sqrt(max of the `count` rows) (one wave; the square root of the largest |r|^2 is the largest |r|)
__global__ __launch_bounds__(64) void k_pgo_max_rows(const double *__restrict__ rows, int count, double *__restrict__ slot) {
  double m = 0;
  for (int r = threadIdx.x; r < count; r += 64) m = fmax(m, rows[r]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
  if (threadIdx.x == 0) slot[0] = sqrt(m);
}

}  // namespace

struct mi_pgo_trans {
  mi_ctx *ctx = nullptr;
  size_t N = 0, E = 0, nslices = 0, padded = 0, anchor = 0;
  DevPtr<long long> slice_ptr;
  DevPtr<int> perm, nbr;
  DevPtr<uint32_t> slot;
  DevPtr<double> tinc, tauinc;
  DevPtr<int2> e_ij;
  DevPtr<double> e_t, e_tau;
  Owned<mi_vec> dinv, b, g, work;  // 3N each: 1 / diagonal; the right-hand side, its negative and L_a t of mi_pgo_trans_solve
  Owned<mi_csr> A;                 // L_a
  Owned<mi_op> L;                  // mi_op_create_csr(ctx, A, 3): lent out as `borrowed`
  Owned<mi_precon> jacobi;         // mi_precon_create_diag(ctx, dinv): lent out as `borrowed`
};

namespace {

#define PGO_REQUIRE_ARGS(cond) MI_REQUIRE(cond, "null argument")
int check_R(const mi_pgo_trans *T, const mi_vec *R) {
  MI_REQUIRE(R->ctx == T->ctx && R->n == 9 * T->N, "R must hold N row-major 3x3 blocks");
  return MI_OK;
}
int check_field(const mi_pgo_trans *T, const mi_vec *t, const char *what) {
  MI_REQUIRE(t->ctx == T->ctx && t->n == 3 * T->N, "%s must hold 3N doubles", what);
  return MI_OK;
}
PgoIncView inc_view(const mi_pgo_trans *T) {
  return PgoIncView{T->nslices, T->slice_ptr.get(), T->perm.get(), T->nbr.get(), T->slot.get(), T->tinc.get(), T->tauinc.get()};
}
int edge_grid(const mi_pgo_trans *T) {
  return (int)std::min<size_t>(std::max<size_t>(1, (T->E + kPgoEdgeBlock - 1) / kPgoEdgeBlock), (size_t)kMaxRows);
}
int launch_rhs(mi_pgo_trans *T, const mi_vec *R, mi_vec *b) {
  mi_ctx *ctx = T->ctx;
  touch(b);
  const int grid = uniform_grid(ctx, (T->nslices + kWaves - 1) / kWaves);
  hipLaunchKernelGGL(k_pgo_trans_rhs, dim3(grid), dim3(kBlock), 0, ctx->stream, inc_view(T), (const double *)R->d, b->d);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
// the residual pass and its two reductions into scalars[slot0], scalars[slot0 + 1] = {f_tau, max |r_e|}; no read-back
int launch_residual(mi_pgo_trans *T, const mi_vec *R, const mi_vec *t, mi_vec *r_out, int slot0) {
  mi_ctx *ctx = T->ctx;
  const int grid = edge_grid(T);
  const PgoEdgeView ev{T->E, T->e_ij.get(), T->e_t.get(), T->e_tau.get()};
  if (r_out) {
    touch(r_out);
    hipLaunchKernelGGL(k_pgo_trans_residual<true>, dim3(grid), dim3(kPgoEdgeBlock), 0, ctx->stream, ev, (const double *)R->d,
                       (const double *)t->d, r_out->d, ctx->partials2);
  } else {
    hipLaunchKernelGGL(k_pgo_trans_residual<false>, dim3(grid), dim3(kPgoEdgeBlock), 0, ctx->stream, ev, (const double *)R->d,
                       (const double *)t->d, (double *)nullptr, ctx->partials2);
  }
  MI_HIP(hipGetLastError());
  MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, grid, 1, ctx->scalars + slot0));
  hipLaunchKernelGGL(k_pgo_max_rows, dim3(1), dim3(64), 0, ctx->stream, (const double *)(ctx->partials2 + kMaxRows), grid,
                     ctx->scalars + slot0 + 1);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_pgo_trans_create(mi_ctx *ctx, size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *tt,
                        const double *tau, long long anchor, mi_pgo_trans **out) {
  MI_REQUIRE(ctx && out && (E == 0 || (ei && ej && tt && tau)), "null argument");
  MI_REQUIRE(!ctx->uniform_grid && !ctx->comm, "the translation recovery of a pose graph is single-context");
  PgoTransPack P;
  std::string err;
  MI_REQUIRE(pgo_trans_pack(N, E, ei, ej, tt, tau, anchor, P, err) == 0, "%s", err.c_str());
  auto T = std::make_unique<mi_pgo_trans>();  // (everything below is owned: an early return releases what was made)
  T->ctx = ctx;
  T->N = N, T->E = E, T->nslices = P.nslices, T->padded = P.padded, T->anchor = P.anchor;
  MI_TRY(dev_upload(T->slice_ptr, P.slice_ptr.data(), P.slice_ptr.size()));
  MI_TRY(dev_upload(T->perm, P.perm.data(), P.perm.size()));
  MI_TRY(dev_upload(T->nbr, P.nbr.data(), P.padded));
  MI_TRY(dev_upload(T->slot, P.slot.data(), P.slot.size()));
  MI_TRY(dev_upload(T->tinc, P.tinc.data(), P.tinc.size()));
  MI_TRY(dev_upload(T->tauinc, P.tauinc.data(), P.tauinc.size()));
  MI_TRY(dev_upload(T->e_ij, reinterpret_cast<const int2 *>(P.e_ij.data()), E));
  MI_TRY(dev_upload(T->e_t, P.e_t.data(), P.e_t.size()));
  MI_TRY(dev_upload(T->e_tau, P.e_tau.data(), P.e_tau.size()));
  MI_TRY(vec_alloc(ctx, 3 * N, T->dinv));
  MI_TRY(mi_vec_upload(T->dinv.get(), P.dinv.data(), 3 * N));
  MI_TRY(vec_alloc(ctx, 3 * N, T->b));
  MI_TRY(vec_alloc(ctx, 3 * N, T->g));
  MI_TRY(vec_alloc(ctx, 3 * N, T->work));
  mi_csr *A = nullptr;
  MI_TRY(mi_csr_create(ctx, N, P.nnz, P.rowptr.data(), P.col.data(), P.val.data(), &A));
  T->A.reset(A);
  mi_op *L = nullptr;
  MI_TRY(mi_op_create_csr(ctx, A, 3, &L));
  T->L.reset(L);
  L->borrowed = true;
  mi_precon *J = nullptr;
  MI_TRY(mi_precon_create_diag(ctx, T->dinv.get(), &J));
  T->jacobi.reset(J);
  J->borrowed = true;
  *out = T.release();
  return MI_OK;
}

int mi_pgo_trans_destroy(mi_pgo_trans *T) {
  if (!T) return MI_OK;
  (void)hipStreamSynchronize(T->ctx->stream);
  delete T;
  return MI_OK;
}

int mi_pgo_trans_rhs(mi_pgo_trans *T, const mi_vec *R, mi_vec *b) {
  PGO_REQUIRE_ARGS(T && R && b);
  MI_TRY(check_R(T, R));
  MI_TRY(check_field(T, b, "b"));
  return launch_rhs(T, R, b);
}

int mi_pgo_trans_operator(mi_pgo_trans *T, mi_op **L, mi_precon **jacobi) {
  PGO_REQUIRE_ARGS(T);
  if (L) *L = T->L.get();
  if (jacobi) *jacobi = T->jacobi.get();
  return MI_OK;
}

int mi_pgo_trans_residual(mi_pgo_trans *T, const mi_vec *R, const mi_vec *t, mi_vec *r_out, double out[2]) {
  PGO_REQUIRE_ARGS(T && R && t && out);
  MI_TRY(check_R(T, R));
  MI_TRY(check_field(T, t, "t"));
  MI_REQUIRE(!r_out || (r_out->ctx == T->ctx && r_out->n == 3 * T->E), "r_out must hold 3E doubles");
  MI_TRY(launch_residual(T, R, t, r_out, SLOT_MISC));
  return read_slots_sync(T->ctx, SLOT_MISC, 2, out);  // the one read-back
}

int mi_pgo_trans_solve(mi_pgo_trans *T, const mi_vec *R, double tol, size_t max_iterations, mi_vec *t_out,
                       mi_pgo_trans_info *info) {
  PGO_REQUIRE_ARGS(T && R && t_out && info);
  MI_TRY(check_R(T, R));
  MI_TRY(check_field(T, t_out, "t_out"));
  MI_REQUIRE(tol >= 0 && tol < 1, "the relative tolerance must lie in [0, 1)");
  mi_ctx *ctx = T->ctx;
  MI_TRY(launch_rhs(T, R, T->b.get()));
  MI_TRY(mi_vec_scale_to(T->g.get(), -1.0, T->b.get()));  // the model 1/2 t'L t + g't with g = -b
  // plain PCG: the radius never binds, theta = 0 and kappa_fgr = tol give the stop sqrt(<r,v>) <= tol sqrt(<r0,v0>)
  mi_stpcg_params prm;
  mi_stpcg_default_params(&prm);
  prm.Delta = kPgoDelta;
  prm.max_iterations = max_iterations;
  prm.kappa_fgr = tol;
  prm.theta = 0.0;
  mi_stpcg_result res;
  MI_TRY(mi_stpcg(ctx, T->g.get(), T->L.get(), T->jacobi.get(), &prm, t_out, &res, nullptr));
  // |L_a t - b| / |b| from one plain application (not the recurrence), and the residual pass: one read-back for both
  MI_TRY(mi_op_apply(T->L.get(), t_out, T->work.get()));
  MI_TRY(mi_vec_axpy(T->work.get(), -1.0, T->b.get()));
  const double *x[2] = {T->work->d, T->b->d};
  MI_TRY(dot_batch_to_slots(ctx, 2, x, x, 3 * T->N, SLOT_MISC + 2));
  MI_TRY(launch_residual(T, R, t_out, nullptr, SLOT_MISC));
  double s[4];
  MI_TRY(read_slots_sync(ctx, SLOT_MISC, 4, s));
  info->iterations = res.num_iterations;
  info->exit_reason = res.exit_reason;
  info->objective = s[0];
  info->max_residual = s[1];
  info->relative_residual = s[3] > 0 ? std::sqrt(s[2]) / std::sqrt(s[3]) : std::sqrt(s[2]);
  return MI_OK;
}

}  // extern "C"
