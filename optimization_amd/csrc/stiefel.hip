// stiefel.hip -- Stiefel manifold St(n,p) (embedded metric) kernels for p <= 8 -- the one-pass Hessian of rows of 5 ... 8
// doubles lives in stiefel_wide.h, rows of 9 ... 16 doubles are routed to the tall-row family of stiefel_tall.hip by the
// entry points below -- and the Rayleigh-quotient
// problem  f(X) = .5 tr(X' A X):  the Objective / QuadraticModel / RiemannianMetric / Retraction
// callables a TNT client supplies (Riemannian/Concepts.h:44-112).  The reference ships only the
// S^2 = St(3,1) lambdas of tests/TNT_unit_test.cpp:73-117; these are their n x p generalisation:
//     project  P_X(Z) = Z - X sym(X'Z)                      (sphere: V - X.dot(V) X,  :73-75)
//     gradient P_X(A X)                                     (:79-85)
//     Hessian  P_X(A V - V sym(X'AX))                       (:94-97)
//     retract  polar factor of X + V                        ((X+V).normalized(),      :106-108)
//
// Per Hessian application (N = n p doubles, A in sliced-ELL) exactly two kernels run:
//   k_st_spmm_gram  reads A, V (gathered through L2), X; writes Z = A V - V S; one partial row of
//                   sym(X'Z) per workgroup                                  [12 nnz + 4 n + 8 (3N)]
//   k_st_finish     prologue: every workgroup re-reduces those <= 512 rows (deterministic);
//                   body: Hp = Z - X sym(X'Z); partial rows of <V,Hp>, <Hp,Hp>, <V,V>      [8 (4N)]
// so the three curvature inner products of STPCG (IterativeSolvers.h:300,305-306) cost no extra pass
// and no scalar kernel sits between the passes.
#include "comm_ipc.h"
#include "spmm_core.h"
#include "stiefel_core.h"
#include "stiefel_tall.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

using namespace mi;

namespace {

enum { POST_SYM = 1, POST_INVSQRT = 2 };

// A scheduling fence behind every column of the P x P products of a wide row (p > 4): without it the scheduler issues
// all 192 LDS reads of a row up front -- 128 more live doubles -- and the kernel loses its second wave per SIMD.
__device__ __forceinline__ void wide_sched() { __builtin_amdgcn_sched_barrier(0); }
// entries per chunk of sell_stream (spmm_core.h CHK) by row width: rows of 7 and 8 doubles gather two at a time
template <int P>
struct StChunk {
  static constexpr int value = P >= 7 ? 2 : kSpmmChunk;
};


// ---- small dense helpers (device) --------------------------------------------------------
template <int P>
__device__ void dev_sym_invsqrt(const double *G, double *out) {
  // cyclic Jacobi on the P x P symmetric matrix G; out = Q diag(w^-1/2) Q'
  double M[P * P], Q[P * P];
  for (int i = 0; i < P * P; ++i) { M[i] = G[i]; Q[i] = 0; }
  for (int i = 0; i < P; ++i) Q[i * P + i] = 1;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int i = 0; i < P; ++i)
      for (int j = i + 1; j < P; ++j) off += M[i * P + j] * M[i * P + j];
    if (off == 0) break;
    for (int i = 0; i + 1 < P; ++i)
      for (int j = i + 1; j < P; ++j) {
        const double apq = M[i * P + j];
        if (apq == 0) continue;
        const double tau = (M[j * P + j] - M[i * P + i]) / (2 * apq);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1 + tau * tau));
        const double c = 1 / sqrt(1 + t * t), s = t * c;
        for (int k = 0; k < P; ++k) {
          const double a = M[k * P + i], b = M[k * P + j];
          M[k * P + i] = c * a - s * b;
          M[k * P + j] = s * a + c * b;
        }
        for (int k = 0; k < P; ++k) {
          const double a = M[i * P + k], b = M[j * P + k];
          M[i * P + k] = c * a - s * b;
          M[j * P + k] = s * a + c * b;
        }
        for (int k = 0; k < P; ++k) {
          const double a = Q[k * P + i], b = Q[k * P + j];
          Q[k * P + i] = c * a - s * b;
          Q[k * P + j] = s * a + c * b;
        }
      }
  }
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j) {
      double acc = 0;
      for (int k = 0; k < P; ++k) acc += Q[i * P + k] * (1.0 / sqrt(M[k * P + k])) * Q[j * P + k];
      out[i * P + j] = acc;
    }
}

// G^-1/2 for rows wider than 4 doubles (r05), by ONE WAVE with the matrices in LDS: the coupled Newton-Schulz iteration
//     Y0 = G / s, Z0 = I;  T = Z Y;  Y <- Y (3 I - T) / 2,  Z <- (3 I - T) Z / 2;   Z -> (G / s)^-1/2,  s = |G|_F
// (eigenvalues of G / s lie in (0, 1], so |I - G / s| < 1: it converges for every SPD G, quadratically; the polar
// retraction's G = (X + V)'(X + V) = I + V'V for a tangent V has its spectrum in [1, s]: log2(s) + ~6 iterations).
// Three 8 x 8 matrix products per iteration, lane (i, j) one entry each: ~1 us per iteration.  dev_sym_invsqrt's
// cyclic Jacobi is strictly serial -- ~300 rotations with three dependent divisions / square roots each, M and Q in
// scratch memory at P = 8: the retraction took 1.7 ms at n = 1e6; as a wave-parallel Jacobi in LDS still 0.65 ms -- and
// stays the p <= 4 path (same rotations as the oracle's).  Here the result agrees with it to rounding (tested at 1e-13).
// T, Y, Z: P x P doubles of LDS each (work[0 .. 3 P P)); out may be LDS.  All 64 lanes of the calling wave call it.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int P>
__device__ void dev_sym_invsqrt_wave(const double *G, double *work, double *out) {
  double *T = work, *Y = work + P * P, *Z = work + 2 * P * P;
  const int l = threadIdx.x & 63, i = (l < P * P ? l : 0) / P, j = (l < P * P ? l : 0) % P;
  const bool mine = l < P * P;
  double s2 = 0;
  for (int k = 0; k < P * P; ++k) s2 += G[k] * G[k];
  const double sc = sqrt(s2);
  if (mine) {
    Y[l] = G[l] / sc;
    Z[l] = (i == j) ? 1.0 : 0.0;
  }
  wave_lds_sync();
  bool last = false;
  for (int it = 0; it < 100; ++it) {
    double t = 0;
    for (int k = 0; k < P; ++k) t += Z[i * P + k] * Y[k * P + j];
    if (mine) T[l] = t;
    wave_lds_sync();
    double err = 0;  // |Z Y - I|_F^2, the same number in every lane
    for (int k = 0; k < P * P; ++k) {
      const double d = T[k] - ((k / P == k % P) ? 1.0 : 0.0);
      err += d * d;
    }
    double yn = 0, zn = 0;
    for (int k = 0; k < P; ++k) {
      const double rkj = ((k == j) ? 3.0 : 0.0) - T[k * P + j], rik = ((i == k) ? 3.0 : 0.0) - T[i * P + k];
      yn += Y[i * P + k] * rkj;
      zn += rik * Z[k * P + j];
    }
    wave_lds_sync();
    if (mine) {
      Y[l] = .5 * yn;
      Z[l] = .5 * zn;
    }
    wave_lds_sync();
    if (last) break;
    if (!(err > 1e-26)) last = true;  // (converged to ~1e-13: one more quadratic step finishes it; NaN ends it too)
  }
  if (mine) out[l] = Z[l] / sqrt(sc);
  wave_lds_sync();
}

// ---- kernels -----------------------------------------------------------------------------

// Z = A V - V S (S may be null => Z = A V); partial row of sym(X'Z)
template <int P>
__global__ __launch_bounds__(kBlock) void k_st_spmm_gram(SellView A, const CgState *__restrict__ st,
                                                         const double *__restrict__ V,
                                                         const double *__restrict__ X,
                                                         const double *__restrict__ S,
                                                         double *__restrict__ Z,
                                                         double *__restrict__ partials) {
  __shared__ double lds[SymIdx<P>::NS * kWaves];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double Sm[P * P];
#pragma unroll
  for (int i = 0; i < P * P; ++i) Sm[i] = S ? S[i] : 0.0;
  double G[P * P];
#pragma unroll
  for (int i = 0; i < P * P; ++i) G[i] = 0;
  const size_t ngroups = (A.nslices + kSlicesPerGroup - 1) / kSlicesPerGroup;
  size_t g0, g1;
  group_range(ngroups, g0, g1);
  for (size_t g = g0; g < g1; ++g) {
    const size_t slice = g * kSlicesPerGroup + w;
    if (slice >= A.nslices) continue;
    const size_t row = slice * 64 + lane;
    double acc[P];
    sell_row_times<P>(A, slice, lane, V, acc);
    if (row < A.n) {
      double x[P], v[P];
#pragma unroll
      for (int c = 0; c < P; ++c) { x[c] = X[row * P + c]; v[c] = V[row * P + c]; }
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int a = 0; a < P; ++a) t += v[a] * Sm[a * P + b];
        acc[b] -= t;
        Z[row * P + b] = acc[b];
      }
#pragma unroll
      for (int a = 0; a < P; ++a)
#pragma unroll
        for (int b = 0; b < P; ++b) G[a * P + b] += x[a] * acc[b];
    }
  }
  store_sym_partials<P>(G, lds, partials);
}

// out = P_X(A V - V S) and the three curvature partials in ONE pass.  The projection's matrix
// M = sym(X'(A V - V S)) is known before the pass: for symmetric A it equals sym(Y'V - (X'V) S) with
// Y = A X fixed during the inner solve, and STPCG's direction kernel left its partial rows when it formed
// V (mi_op::dirgram).  So no second pass over Z, X, V is needed (k_st_finish: 8 (4N) bytes saved).
// k_st_spmm_gram on the lean pipelined core (packed matrix when there is one); same arithmetic per row
template <int P, bool HALO, bool PK>
__global__ __launch_bounds__(StBlk<P>::threads) void k_st_spmm_gram_stream(SellView A, const CgState *__restrict__ st,
                                                                const double *__restrict__ V,
                                                                const double *__restrict__ X,
                                                                const double *__restrict__ S,
                                                                double *__restrict__ Z,
                                                                double *__restrict__ partials) {
  constexpr int NW = StBlk<P>::waves;
  constexpr bool WIDE = P > 4;  // (rows wider than 4 doubles: 256-thread workgroups, S in LDS: stiefel_core.h StBlk)
  __shared__ double lds[SymIdx<P>::NS * NW];
  __shared__ double vt[PK ? 256 : 1];
  __shared__ double SmL[WIDE ? P * P : 1];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (PK) {
    if (threadIdx.x < 256) vt[threadIdx.x] = A.vtab[threadIdx.x];
  }
  if (WIDE && threadIdx.x < P * P) SmL[threadIdx.x] = S ? S[threadIdx.x] : 0.0;
  if (PK || WIDE) __syncthreads();
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t s0 = (A.nslices * lb) / nb, s1 = (A.nslices * (lb + 1)) / nb;
  double SmR[WIDE ? 1 : P * P];
  if (!WIDE) {
#pragma unroll
    for (int i = 0; i < P * P; ++i) SmR[i] = S ? S[i] : 0.0;
  }
  double G[P * P];
#pragma unroll
  for (int i = 0; i < P * P; ++i) G[i] = 0;
  struct Epi {
    const SellView &A;
    const double *__restrict__ X, *__restrict__ V;
    double *__restrict__ Z;
    const double (&SmR)[WIDE ? 1 : P * P];  // S in registers (p <= 4) ...
    const double *SmL;                      // ... or in LDS
    double (&G)[P * P];
    int lane;
    double x[P], v[P];
    __device__ __forceinline__ unsigned lane_off(size_t slice) const {
      return (slice * 64 + lane < A.n) ? (unsigned)lane * (unsigned)(P * 8) : 0u;
    }
    __device__ __forceinline__ void begin(size_t slice) {
      const unsigned off = lane_off(slice);
      const double *xs = reinterpret_cast<const double *>(reinterpret_cast<const char *>(X + slice * 64 * P) + off);
      const double *vs = reinterpret_cast<const double *>(reinterpret_cast<const char *>(V + slice * 64 * P) + off);
#pragma unroll
      for (int c = 0; c < P; ++c) { x[c] = xs[c]; v[c] = vs[c]; }
    }
    __device__ __forceinline__ void end(size_t slice, double (&acc)[P]) {
      if (slice * 64 + lane >= A.n) return;
      if (WIDE) asm volatile("" ::: "memory");  // (S is re-read from LDS per row, not parked in 64 registers)
      double *zs = reinterpret_cast<double *>(reinterpret_cast<char *>(Z + slice * 64 * P) + lane_off(slice));
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int a = 0; a < P; ++a) t += v[a] * (WIDE ? SmL[a * P + b] : SmR[WIDE ? 0 : a * P + b]);
        acc[b] -= t;
        zs[b] = acc[b];
        if (WIDE) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int a = 0; a < P; ++a)
#pragma unroll
        for (int b = 0; b < P; ++b) G[a * P + b] += x[a] * acc[b];
    }
  } epi{A, X, V, Z, SmR, SmL, G, lane, {}, {}};
  sell_stream<P, HALO, PK, Epi, NW, StChunk<P>::value>(
      A, s0 + (size_t)__builtin_amdgcn_readfirstlane(w), s1, lane, V, vt, epi);
  store_sym_partials<P>(G, lds, partials);
}

// RECUR (mi_op::apply_dir with gram_count < 0): M is read from gdir (packed symmetric, replicated scalars kept
// by STPCG) and the packed symmetric Gram  sym(Y'out - (X'out) S)  of the OUTPUT rides along as components
// 3.. of the partial row (DirComps<P>::value components in all).
// HW > 0 (mi_csr::win_chunks > 0): the window form -- the rows of V near the workgroup's own are staged in an LDS
// ring and every entry's row is read from LDS at an address the host worked out (spmm_core.h sell_window); HW = the
// entries per slice.  Same arithmetic, bit-identical results.
// FAR (window form, unsharded): 0 far columns loaded; 1 computed (pure far structure); 2 computed + 16-bit words
// TWOK (r05, opt-in experiment TWO_KERNEL_STEP, window form only): the pass also reads the residual r and leaves the
// partial rows of <r,out> and <V,r> (components KC-2, KC-1): with them <r+,r+> = <r,r> + 2 alpha <r,Hp> + alpha^2 <Hp,Hp>
// is known without a pass over r+, and the two CG kernels of an iteration merge into one (stpcg.hip k_cg_step2).
template <int P, bool FROM_SLOTS, bool HALO, bool RECUR, bool PK, int HW, int FAR = 0, bool TWOK = false>
__global__ __launch_bounds__(HW > 0 ? kWinBlock : kBlock) void k_st_hess_fused(SellView A, WinView Wv, const CgState *__restrict__ st,
                                                          const double *__restrict__ V,
                                                          const double *__restrict__ X,
                                                          const double *__restrict__ Y,
                                                          const double *__restrict__ S,
                                                          const double *__restrict__ gram_partials, int count,
                                                          const double *__restrict__ slots,
                                                          const double *__restrict__ gdir,
                                                          double *__restrict__ out,
                                                          double *__restrict__ partials, HaloWaitArg<HALO> hwait,
                                                          const double *__restrict__ Rres = nullptr) {
  constexpr bool WIN = HW > 0 && P <= 3;  // (P = 4: ring + parked rows would need > 160 KB of LDS; never dispatched)
  static_assert(!TWOK || (WIN && RECUR), "the two-kernel step exists in the window form only");
  constexpr int NS = SymIdx<P>::NS, KC = TWOK ? 3 + NS + 2 : (RECUR ? DirComps<P>::value : 3);
  constexpr int kLds = (NS * (kWaves + 1) > KC * kWaves) ? NS * (kWaves + 1) : KC * kWaves;
  __shared__ double lds[kLds];
  __shared__ double vt[PK ? 256 : 1];  // PK: the matrix's value table
  __shared__ double ring[WIN ? kWinLdsRows * P : 1];  // WIN: ring, zero row, far slots
  if (st && st->mode != CG_RUN) return;
  // sharded: the neighbours' rows of V were pushed by the kernel that wrote V (comm_ipc.h HaloPush); wait for them here
  if constexpr (HALO) halo_wait(hwait.w);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#ifdef MI_WIN_STAMPS  // both forms: each wave's entry and exit on the constant 100 MHz clock (slots 56, 57)
  const unsigned long long t_entry = wall_clock64();
#endif
  if (PK) {
    if (threadIdx.x < 256) vt[threadIdx.x] = A.vtab[threadIdx.x];
    if (!WIN) __syncthreads();  // WIN: the barrier behind the ring fill publishes the table too
  }
  // a contiguous range of SLICES per workgroup (XCD-aware like group_range, but balanced to one slice)
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t s0 = (A.nslices * lb) / nb, s1 = (A.nslices * (lb + 1)) / nb;
  double Sm[P * P];
#pragma unroll
  for (int i = 0; i < P * P; ++i) Sm[i] = S[i];
  double Mm[P * P];
  if (RECUR) {
#pragma unroll
    for (int aa = 0; aa < P; ++aa)
#pragma unroll
      for (int b = aa; b < P; ++b) {
        const double m = gdir[SLOT_GDIR_P + SymIdx<P>::at(aa, b)];
        Mm[aa * P + b] = m;
        Mm[b * P + aa] = m;
      }
  } else {
    load_sym<P, FROM_SLOTS>(gram_partials, count, slots, Mm, lds);
  }
  double a[KC];
#pragma unroll
  for (int i = 0; i < KC; ++i) a[i] = 0;
  struct Epi {
    const SellView &A;
    const double *__restrict__ X, *__restrict__ Y, *__restrict__ V;
    double *__restrict__ out;
    const double (&Sm)[P * P], (&Mm)[P * P];
    double (&a)[KC];
    int lane;
    double x[P], y[P], v[P];
    const double *__restrict__ Rr;
    double rr[TWOK ? P : 1], rn[TWOK ? P : 1];
    // rows of the slice from a scalar base + a 32-bit lane offset (lanes past the last row read its first)
    // (32-bit arithmetic: the fields span < 4 GiB, sell_stream_ok)
    __device__ __forceinline__ unsigned lane_off(size_t slice) const {
      return ((unsigned)slice * 64u + (unsigned)lane < (unsigned)A.n) ? (unsigned)lane * (unsigned)(P * 8) : 0u;
    }
    __device__ __forceinline__ const double *row_of(const double *F, size_t slice, unsigned off) const {
      return reinterpret_cast<const double *>(reinterpret_cast<const char *>(F) + (unsigned)slice * (unsigned)(64 * P * 8) +
                                              off);
    }
    __device__ __forceinline__ void begin(size_t slice) {
      const unsigned off = lane_off(slice);
      const double *xs = row_of(X, slice, off);
#pragma unroll
      for (int c = 0; c < P; ++c) x[c] = xs[c];
      if (!WIN) {  // WIN: the row of V comes from the ring (end(slice, acc, vrow))
        const double *vs = row_of(V, slice, off);
#pragma unroll
        for (int c = 0; c < P; ++c) v[c] = vs[c];
      }
      if (RECUR) {
        const double *ys = row_of(Y, slice, off);
#pragma unroll
        for (int c = 0; c < P; ++c) y[c] = ys[c];
      }
    }
    // sell_window's protocol: request(slice) issues the loads of the slice's rows (pinned: see spmm_core.h),
    // end(slice, acc, vrow) consumes them
    double xn[WIN ? P : 1], yn[WIN ? P : 1];
    __device__ __forceinline__ void request(size_t slice) {
      const unsigned off = lane_off(slice);
      const double *xs = row_of(X, slice, off);
#pragma unroll
      for (int c = 0; c < P; ++c) xn[WIN ? c : 0] = pinned_load(xs + c);
      if (RECUR) {
        const double *ys = row_of(Y, slice, off);
#pragma unroll
        for (int c = 0; c < P; ++c) yn[WIN ? c : 0] = pinned_load(ys + c);
      }
      if (TWOK) {
        const double *rs = row_of(Rr, slice, off);
#pragma unroll
        for (int c = 0; c < P; ++c) rn[TWOK ? c : 0] = pinned_load(rs + c);
      }
    }
    __device__ __forceinline__ void end(size_t slice, double (&acc)[P], const double (&vrow)[P]) {
#pragma unroll
      for (int c = 0; c < P; ++c) {
        v[c] = vrow[c];
        x[c] = xn[WIN ? c : 0];
        if (RECUR) y[c] = yn[WIN ? c : 0];
        if (TWOK) rr[TWOK ? c : 0] = rn[TWOK ? c : 0];
      }
      end(slice, acc);
    }
    __device__ __forceinline__ void end(size_t slice, double (&acc)[P]) {
      if ((unsigned)slice * 64u + (unsigned)lane >= (unsigned)A.n) return;
      double *os = reinterpret_cast<double *>(reinterpret_cast<char *>(out) + (unsigned)slice * (unsigned)(64 * P * 8) +
                                              lane_off(slice));
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += v[aa] * Sm[aa * P + b];
        acc[b] -= t;  // Z = A V - V S
      }
      double o[P];
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += x[aa] * Mm[aa * P + b];
        o[b] = acc[b] - t;  // Z - X M
        os[b] = o[b];
        a[0] += v[b] * o[b]; a[1] += o[b] * o[b]; a[2] += v[b] * v[b];
        if (TWOK) { a[KC - 2] += rr[TWOK ? b : 0] * o[b]; a[KC - 1] += v[b] * rr[TWOK ? b : 0]; }
      }
      if (RECUR) {  // packed sym(y o' - x (o S)'): the Gram of this output row
        double os_[P];
#pragma unroll
        for (int b = 0; b < P; ++b) {
          double t = 0;
#pragma unroll
          for (int aa = 0; aa < P; ++aa) t += o[aa] * Sm[aa * P + b];
          os_[b] = t;
        }
#pragma unroll
        for (int aa = 0; aa < P; ++aa)
#pragma unroll
          for (int b = aa; b < P; ++b) {
            const double gab = y[aa] * o[b] - x[aa] * os_[b];
            const double gba = y[b] * o[aa] - x[b] * os_[aa];
            a[3 + SymIdx<P>::at(aa, b)] += (aa == b) ? gab : .5 * (gab + gba);
          }
      }
    }
  } epi{A, X, Y, V, out, Sm, Mm, a, lane, {}, {}, {}, Rres, {}, {}, {}, {}};
  // the wave index as a scalar: slice bounds then come from scalar loads and the loop control is scalar
  const int wu = __builtin_amdgcn_readfirstlane(w);
  if constexpr (WIN) {
    // a contiguous run of whole TILES (kWinWaves slices) per workgroup: the launch plan's table, or equal runs
    const int ntiles = (int)((A.nslices + kWinWaves - 1) / kWinWaves), per = (ntiles + (int)nb - 1) / (int)nb;
    int t0 = (int)lb * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    if (Wv.bounds) {  // runs cut to the stride of the far entries (window_bounds)
      t0 = scalar_int(Wv.bounds, lb);
      t1 = scalar_int(Wv.bounds, lb + 1);
    }
    if constexpr (HALO)
      sell_window<P, HW, true, (FAR >= 1), false>(A, Wv, t0, t1, wu, lane, V, vt, ring, epi, hwait.halo_lo, hwait.halo_hi);
    else
      // (FARC = false: far rows as coalesced images change nothing at p <= 3, the gathers stay -- EXPERIMENTS.md "Decided knobs")
      sell_window<P, HW, false, (FAR >= 1), (FAR == 2), Epi, P, false>(A, Wv, t0, t1, wu, lane, V, vt, ring, epi);
  } else {
    sell_stream<P, HALO, PK>(A, s0 + (size_t)wu, s1, lane, V, vt, epi);
  }
#ifdef MI_WIN_STAMPS
  const unsigned long long t_body = wall_clock64();
#endif
  if constexpr (WIN) block_partials_store_nw<KC, kWinWaves>(a, lds, partials);
  else block_partials_store<KC>(a, lds, partials);
#ifdef MI_WIN_STAMPS
  if (g_stamp_buf && lane == 0) {
    unsigned long long *o = g_stamp_buf + ((size_t)blockIdx.x * (WIN ? kWinWaves : kWaves) + w) * kStampSlots;
    o[56] = t_entry;
    o[57] = wall_clock64();
    o[58] = t_body;
  }
#endif
}

#include "stiefel_wide.h"  // rows wider than 4 doubles (p = 5 ... 8): k_st_hess_wide, k_st_hess_widewin, k_st_hess_wideq

// Gram partial rows of two dense n x P fields.
//   VARIANT 0: gram(X,Z)              1: Y = X + Z written to out, gram(Y,Y)
//           2: Z' = dinv_rows .* Z written to out, gram(X,Z')
//   SYM: symmetrised partials (P(P+1)/2 components) else raw (P*P components)
template <int P, int VARIANT, bool SYM>
__global__ __launch_bounds__(StBlk<P>::threads) void k_st_gram(size_t n, const double *__restrict__ X,
                                                    const double *__restrict__ Zin,
                                                    const double *__restrict__ dinv,
                                                    double *__restrict__ out,
                                                    double *__restrict__ partials) {
  constexpr int BLK = StBlk<P>::threads, NW = StBlk<P>::waves;
  __shared__ double lds[P * P * NW];
  double G[P * P];
#pragma unroll
  for (int i = 0; i < P * P; ++i) G[i] = 0;
  const size_t stride = (size_t)gridDim.x * BLK;
  for (size_t row = (size_t)blockIdx.x * BLK + threadIdx.x; row < n; row += stride) {
    double x[P], z[P];
#pragma unroll
    for (int c = 0; c < P; ++c) { x[c] = X[row * P + c]; z[c] = Zin[row * P + c]; }
    if (VARIANT == 1) {
#pragma unroll
      for (int c = 0; c < P; ++c) { x[c] = x[c] + z[c]; z[c] = x[c]; out[row * P + c] = x[c]; }
    } else if (VARIANT == 2) {
      const double d = dinv[row];
#pragma unroll
      for (int c = 0; c < P; ++c) { z[c] = d * z[c]; out[row * P + c] = z[c]; }
    }
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
      for (int b = 0; b < P; ++b) G[a * P + b] += x[a] * z[b];
  }
  if (SYM) store_sym_partials<P>(G, lds, partials);
  else block_partials_store_w<P * P, NW>(G, lds, partials);
}

// prologue: M = sym Gram (re-reduced by every workgroup, or read from all-reduced slots);
// body: out = Z - X M;  DOTS: partial rows of <Vin,out>, <out,out>, <Vin,Vin>;  M_out (nullable): M
template <int P, bool DOTS, bool FROM_SLOTS>
__global__ __launch_bounds__(StBlk<P>::threads) void k_st_finish(size_t n, const CgState *__restrict__ st,
                                                      const double *__restrict__ X,
                                                      const double *__restrict__ Z,
                                                      const double *__restrict__ Vin,
                                                      const double *__restrict__ gram_partials, int count,
                                                      const double *__restrict__ slots,
                                                      double *__restrict__ M_out,
                                                      double *__restrict__ out,
                                                      double *__restrict__ partials) {
  constexpr int BLK = StBlk<P>::threads, NW = StBlk<P>::waves;
  constexpr bool WIDE = P > 4;  // (256-thread workgroups, M in LDS: stiefel_core.h StBlk)
  __shared__ double lds[SymIdx<P>::NS * (kWaves + 1) + 3 * kWaves];
  __shared__ double MmL[WIDE ? P * P : 1];
  if (st && st->mode != CG_RUN) return;
  const size_t stride = (size_t)gridDim.x * BLK;
  const size_t row0 = (size_t)blockIdx.x * BLK + threadIdx.x;
  // prefetch the first grid-stride step before the prologue's reduction (hides its latency)
  double x[P], z[P], vi[P];
#pragma unroll
  for (int c = 0; c < P; ++c) { x[c] = 0; z[c] = 0; vi[c] = 0; }
  if (row0 < n) {
#pragma unroll
    for (int c = 0; c < P; ++c) {
      x[c] = X[row0 * P + c];
      z[c] = Z[row0 * P + c];
      if (DOTS) vi[c] = Vin[row0 * P + c];
    }
  }
  double Mm[P * P];
  load_sym<P, FROM_SLOTS>(gram_partials, count, slots, Mm, lds);
  if (M_out && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < P * P; ++i) M_out[i] = Mm[i];
  }
  if (WIDE) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < P * P; ++i) MmL[i] = Mm[i];
    }
    __syncthreads();
  }
  double a[3] = {0, 0, 0};
  for (size_t row = row0; row < n;) {
    const size_t rnext = row + stride;
    double xn[P], zn[P], vn[P];
#pragma unroll
    for (int c = 0; c < P; ++c) { xn[c] = x[c]; zn[c] = z[c]; vn[c] = vi[c]; }
    if (rnext < n) {
#pragma unroll
      for (int c = 0; c < P; ++c) {
        xn[c] = X[rnext * P + c];
        zn[c] = Z[rnext * P + c];
        if (DOTS) vn[c] = Vin[rnext * P + c];
      }
    }
    if (WIDE) asm volatile("" ::: "memory");  // (M is re-read from LDS per row, not parked in 64 registers)
#pragma unroll
    for (int b = 0; b < P; ++b) {
      double t = 0;
#pragma unroll
      for (int aa = 0; aa < P; ++aa) t += x[aa] * (WIDE ? MmL[aa * P + b] : Mm[aa * P + b]);
      const double o = z[b] - t;
      out[row * P + b] = o;
      if (DOTS) { a[0] += vi[b] * o; a[1] += o * o; a[2] += vi[b] * vi[b]; }
      if (WIDE) wide_sched();
    }
    row = rnext;
#pragma unroll
    for (int c = 0; c < P; ++c) { x[c] = xn[c]; z[c] = zn[c]; vi[c] = vn[c]; }
  }
  if (DOTS) block_partials_store_w<3, NW>(a, lds, partials);
}

// retraction finish: Y <- Y (Y'Y)^-1/2, the P x P inverse square root computed once per workgroup
template <int P, bool FROM_SLOTS>
__global__ __launch_bounds__(StBlk<P>::threads) void k_st_polar(size_t n, double *__restrict__ Y,
                                                     const double *__restrict__ gram_partials, int count,
                                                     const double *__restrict__ slots) {
  constexpr int BLK = StBlk<P>::threads;
  constexpr bool WIDE = P > 4;
  __shared__ double lds[SymIdx<P>::NS * (kWaves + 1)];
  __shared__ double Minv[P * P];
  __shared__ double jac[WIDE ? 4 * P * P : 1];  // WIDE: the Gram and the three work matrices of dev_sym_invsqrt_wave
  double G[P * P];
  load_sym<P, FROM_SLOTS>(gram_partials, count, slots, G, lds);
  if (WIDE) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < P * P; ++i) jac[i] = G[i];
    }
    __syncthreads();
    if (threadIdx.x < 64) dev_sym_invsqrt_wave<P>(jac, jac + P * P, Minv);
  } else {
    if (threadIdx.x == 0) dev_sym_invsqrt<P>(G, Minv);
  }
  __syncthreads();
  double Mm[WIDE ? 1 : P * P];
  if (!WIDE) {
#pragma unroll
    for (int i = 0; i < P * P; ++i) Mm[i] = Minv[i];
  }
  const size_t stride = (size_t)gridDim.x * BLK;
  for (size_t row = (size_t)blockIdx.x * BLK + threadIdx.x; row < n; row += stride) {
    double y[P];
#pragma unroll
    for (int c = 0; c < P; ++c) y[c] = Y[row * P + c];
    if (WIDE) asm volatile("" ::: "memory");
#pragma unroll
    for (int b = 0; b < P; ++b) {
      double t = 0;
#pragma unroll
      for (int a = 0; a < P; ++a) t += y[a] * (WIDE ? Minv[a * P + b] : Mm[WIDE ? 0 : a * P + b]);
      Y[row * P + b] = t;
    }
  }
}

// ---- launch helpers (dispatch on p: DISPATCH_P, DISPATCH_P4 of mi_internal.h) ---------------
inline int row_grid(const mi_ctx *ctx, size_t n) { return grid_for(ctx, n, 2); }
// rows wider than 4 doubles run 256-thread workgroups (StBlk): up to kMaxRows of them (one partial row each)
inline int row_grid(const mi_ctx *ctx, size_t n, int p) {
  if (p <= 4 || ctx->uniform_grid) return row_grid(ctx, n);
  size_t blocks = std::max<size_t>(1, (n + 511) / 512);
  blocks = std::min<size_t>(blocks, std::min<size_t>(kMaxRows, 2 * (size_t)ctx->max_grid));
  return (int)blocks;
}
inline int nsym(int p) { return p * (p + 1) / 2; }

// sharded only: partial rows -> slots -> all-reduce
int sharded_reduce(mi_ctx *ctx, int count, int k, double *slots) {
  return reduce_rows_allreduce(ctx, ctx->partials2, count, k, slots);
}

int launch_spmm_gram(mi_ctx *ctx, const mi_csr *A, int p, const CgState *st, const double *V,
                     const double *X, const double *S, double *Z, int *count) {
  if (tall_p(p)) return tall_spmm_gram(ctx, A, p, st, V, X, S, Z, count);  // rows of 9 ... 16 doubles
  const size_t ngroups = sell_groups(A);
  int grid = uniform_grid(ctx, ngroups);
  MI_TRY(comm_halo_exchange(ctx, A, p, V));
  SellView view = sell_view(A);  // after the exchange: it selects the halo buffer the rows landed in
  KScope ks(ctx, MI_K_STIEFEL_SPMM_GRAM);
  const bool no_stream = ctx->cfg.no_spmm_stream;
  // (rows wider than 4 doubles exist in the pipelined form only: 256-thread workgroups, stiefel_core.h StBlk)
  MI_REQUIRE(p <= 4 || sell_stream_ok(A, p), "Stiefel rows of %d doubles need fields below 4 GiB", p);
  if ((!no_stream || p > 4) && sell_stream_ok(A, p)) {
    if (!ctx->uniform_grid && grid > 256) grid = 256;  // one workgroup per CU, one round
    if (p > 4 && !ctx->uniform_grid)                   // 256-thread workgroups: two per CU
      grid = (int)std::max<size_t>(1, std::min<size_t>((A->nslices + 3) / 4, std::min<size_t>(2 * (size_t)ctx->num_cu, 2 * (size_t)ctx->max_grid)));
    DISPATCH_FLAG(A->halo != nullptr, HL, DISPATCH_FLAG(A->pk != nullptr, PK, DISPATCH_P(p,
        hipLaunchKernelGGL((k_st_spmm_gram_stream<P, HL, PK>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, view, st,
                           V, X, S, Z, ctx->partials2))));
  } else {
    DISPATCH_P4(p, hipLaunchKernelGGL(k_st_spmm_gram<P>, dim3(grid), dim3(kBlock), 0, ctx->stream, view, st, V,
                                      X, S, Z, ctx->partials2));
  }
  *count = grid;
  return MI_OK;
}

// out = Z - X sym(Gram) where the symmetrised Gram partial rows are in ctx->partials2
int launch_finish(mi_ctx *ctx, size_t n, int p, const CgState *st, const double *X, const double *Z,
                  const double *Vin, int count, double *M_out, double *out, bool dots, int *nparts) {
  // rows of 9 ... 16 doubles (count = 0: the Gram rows are reduced already, tall_reduce)
  if (tall_p(p)) return tall_finish(ctx, n, p, st, X, Z, Vin, count, M_out, out, dots, nparts);
  const int grid = row_grid(ctx, n, p);
  double *slots = ctx->scalars + SLOT_GRAM;
  // several ranks: all-reduce the Gram partial rows themselves and keep the prologue re-reduction
  // (no one-workgroup reduce kernel); the slot variant stays reachable through MI355OPT_FORCE_SLOT_PATH
  const bool sharded = slot_mode(ctx);
  if (rows_mode(ctx)) MI_TRY(comm_allreduce_rows(ctx, ctx->partials2, nsym(p)));
  if (sharded) MI_TRY(sharded_reduce(ctx, count, nsym(p), slots));
  KScope ks(ctx, MI_K_STIEFEL_FINISH_DOTS);
  DISPATCH_FLAG(dots, D, DISPATCH_FLAG(sharded, F, DISPATCH_P(p,
      hipLaunchKernelGGL((k_st_finish<P, D, F>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, n, st, X, Z, Vin,
                         (const double *)ctx->partials2, count, (const double *)slots, M_out, out, ctx->partials))));
  if (nparts) *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int check_np(mi_ctx *ctx, size_t n, int p, const mi_vec *a, const mi_vec *b, const mi_vec *c) {
  MI_REQUIRE(ctx, "ctx is null");
  MI_REQUIRE(p >= 1 && p <= kMaxPTall, "p must be in [1,%d], got %d", kMaxPTall, p);
  if (tall_p(p)) MI_TRY(tall_check(ctx, nullptr, n, p));  // (one context, fields below 4 GiB)
  const mi_vec *vs[3] = {a, b, c};
  for (const mi_vec *v : vs) {
    if (!v) continue;
    MI_REQUIRE(v->ctx == ctx, "vector belongs to another context");
    MI_REQUIRE(v->n == n * (size_t)p, "expected an n x p = %zu x %d field, got %zu doubles", n, p, v->n);
  }
  return MI_OK;
}

}  // namespace

struct mi_stiefel_rq {
  mi_ctx *ctx;
  const mi_csr *A;
  size_t n;
  int p;
  double *S_dev;  // P*P: sym(X'AX) of the last model() call
  mi_vec *Z;      // n x p scratch
  mi_vec *Y;      // A X of the last model() call (fixed during the inner solve; mi_op::dirgram)
  mi_dirgram dg;
  mi_op hess;     // borrowed operator object bound to X
  const mi_vec *X;
  uint64_t X_serial = 0;  // ("bound to this X": mi::bound_to(X, X_serial, .))
  // mi_stiefel_rq_trial: what it already worked out at the trial point (A X+, sym(X+'A X+), the gradient), handed
  // to the next mi_stiefel_rq_model call if that call is for the same vector with the same contents
  double *S_next = nullptr;
  mi_vec *Y_next = nullptr, *grad_next = nullptr, *Hh = nullptr;
  VecKey trial;
  bool warned_unsymmetric = false;
};

namespace {

int rq_apply_common(mi_op *self, const mi_vec *in, mi_vec *out, bool dots, int *nparts) {
  mi_stiefel_rq *q = (mi_stiefel_rq *)self->impl;
  mi_ctx *ctx = q->ctx;
  int count = 0;
  MI_TRY(launch_spmm_gram(ctx, q->A, q->p, ctx->cg_live, in->d, q->X->d, q->S_dev, q->Z->d, &count));
  return launch_finish(ctx, q->n, q->p, ctx->cg_live, q->X->d, q->Z->d, in->d, count, nullptr, out->d, dots,
                       nparts);
}
int rq_apply(mi_op *self, const mi_vec *in, mi_vec *out) {
  return rq_apply_common(self, in, out, false, nullptr);
}
int rq_apply_dots(mi_op *self, const mi_vec *in, mi_vec *out, int *nparts) {
  return rq_apply_common(self, in, out, true, nparts);
}

// ---- one-pass Hessian for STPCG: the direction kernel left `gram_count` partial rows of sym(Y'in - (X'in) S) ----
// A plan (which of the five kernel forms runs and with which template selectors: plain facts in, no HIP call), the
// kernel a plan names, and one function that enqueues it.
enum StHessForm {
  ST_HESS_PLAIN = 0,    // k_st_hess_fused<P, ., ., ., ., 0>: the streaming form of rows of <= 4 doubles
  ST_HESS_WINDOW = 1,   // k_st_hess_fused<P, false, ., true, true, HW, FAR>: its LDS-window form (p <= 3)
  ST_HESS_WIDEWIN = 2,  // k_st_hess_widewin<P, HW, FARD>: the window form of rows of 4 ... 8 doubles
  ST_HESS_WIDE = 3,     // k_st_hess_wide<P, HALO, PK>: rows of 5 ... 8 doubles, one lane per row
  ST_HESS_WIDEQ = 4     // k_st_hess_wideq<P, HALO, PK>: the same in the quad layout (4 lanes per row)
};

// what the plan reads of a matrix and of its context
struct StHessTraits {
  bool pk, wk, wk16;  // the matrix has a packed copy, window words, their 16-bit form
  int win_chunks, win_head;
  size_t win_far_pure, win_far_stride;
  bool halo, row_sharded;  // a halo buffer exists; csr_row_sharded
  bool no_window, no_far_computed, words16, no_win_bounds, uniform_grid, slot_mode, twok_r;
  int wide_quad, wide_window;
};
// `two_kernel_step`: the context has opted into the two-kernel step (Config::two_kernel_step).  That experiment's Hessian
// pass exists for 4-byte words only, so such a context keeps them; the 16-bit words are every other context's default.
StHessTraits st_hess_traits(const mi_ctx *ctx, const mi_csr *A, bool two_kernel_step) {
  const Config &c = ctx->cfg;
  return {A->pk != nullptr, A->wk != nullptr, A->wk16 != nullptr, A->win_chunks, A->win_head, A->win_far_pure,
          A->win_far_stride, A->halo != nullptr, csr_row_sharded(A), c.no_window, c.no_far_computed,
          c.words16 && !two_kernel_step, c.no_win_bounds, ctx->uniform_grid, slot_mode(ctx), ctx->twok_r != nullptr,
          c.wide_quad, c.wide_window};
}
StHessTraits st_hess_traits(const mi_ctx *ctx, const mi_csr *A) {
  return st_hess_traits(ctx, A, ctx->cfg.two_kernel_step);
}

struct StHessPlan {
  int form = ST_HESS_PLAIN;
  // template selectors of the form's kernel (what a form does not have stays false / 0)
  bool from_slots = false, halo = false, recur = false, pk = false, twok = false;
  int hw = 0;   // entries per slice of the window forms (7 or 8); 0: no window
  int far = 0;  // far columns of the window forms: 0 loaded, 1 computed, 2 computed + 16-bit words
  int block = kBlock;
  size_t lds_bytes = 0;  // dynamic LDS
  int wc = 0;            // window half-width in chunks as the kernel is told (WinView)
  bool fard = false;     // computed far columns (WinView::far_d)
  bool run_table = false;    // the launch asks window_bounds for planned runs
  bool exchange = false;     // comm_halo_exchange_or_wait precedes the launch
  bool gram_reduce = false;  // the Gram rows are reduced first: across ranks in rows mode, into slots where from_slots
  const char *error = nullptr;  // why there is no plan (the function then returns MI_ERR_INVALID_ARGUMENT)
};

int st_hess_plan(int p, int gram_count, const StHessTraits &t, StHessPlan *out) {
  StHessPlan &pl = *out = StHessPlan();
  const auto fail = [&](const char *why) { pl.error = why; return (int)MI_ERR_INVALID_ARGUMENT; };
  if (p < 1 || p > kMaxP) return fail("internal: the one-pass Hessian exists for rows of 1 ... 8 doubles");
  pl.fard = far_computed(t.win_far_pure, t.no_far_computed);
  const int hw = t.win_head <= 7 ? 7 : 8;
  // r06: the wide rows' window form where the matrix has one (packed, window of <= 2 chunks, no halo, one context) --
  // p = 4 ... 7 by default (at p = 8 the ring's rows are 64 bytes apart: 16-way LDS bank conflicts, and the quad layout
  // is there); MI355OPT_WIDE_WINDOW = 0 / 1 forces it off / on for every width
  const bool wide_window = (t.wide_window < 0 ? p <= 7 && !(t.wide_quad > 0) : t.wide_window != 0) && t.pk && t.wk &&
                           t.win_chunks > 0 && t.win_chunks <= 2 && !t.halo && !t.uniform_grid && !t.no_window &&
                           !t.row_sharded;
  // p = 5 ... 8: the recurrence form through k_st_hess_wide / k_st_hess_wideq / k_st_hess_widewin.  p = 4 has no window
  // form of its own (ring + far slots of 4 x 4 workgroups: see WIN in k_st_hess_fused); in the recurrence form it takes
  // the wide rows' (k_st_hess_widewin<4>, dynamic LDS sized for the matrix's own window) where that one applies
  if (p > 4 || (p == 4 && gram_count == -1 && wide_window)) {
    if (gram_count >= 0) return fail("internal: rows wider than 4 doubles take the one-pass Hessian in its recurrence form only");
    pl.recur = true;
    if (wide_window) {
      pl.form = ST_HESS_WIDEWIN, pl.block = kWinBlock, pl.run_table = true;
      pl.pk = true, pl.hw = hw, pl.far = pl.fard ? 1 : 0, pl.wc = t.win_chunks;
      pl.lds_bytes = (size_t)((2 * kWinWaves + 2 * pl.wc) * 64 + 1 + kWinFarRows) * (size_t)(p == 8 ? 9 : p) * sizeof(double);
      return MI_OK;
    }
    // the quad layout where it measured faster (St(1e6,p), profiles/r05_wide_quad_ab.txt: p = 8: 82 vs 98 us; p = 5, 6, 7:
    // 80 / 73 / 93 vs 59 / 69 / 83 us for one lane per row); MI355OPT_WIDE_QUAD=0 / 1 forces either form
    const bool quad = t.wide_quad < 0 ? p == 8 : t.wide_quad != 0;
    pl.form = quad ? ST_HESS_WIDEQ : ST_HESS_WIDE, pl.block = kWideBlock, pl.exchange = true;
    pl.halo = t.halo, pl.pk = t.pk;
    // (runs cut to the far stride; tiles = 4 slices)
    pl.run_table = !t.uniform_grid && t.win_far_stride && !t.no_win_bounds && kWideWaves == kWinWaves;
    return MI_OK;
  }
  pl.recur = gram_count < 0, pl.halo = t.halo, pl.exchange = true, pl.gram_reduce = !pl.recur;
  // the window form when the matrix qualifies (decided at creation, sparse.hip build_window); p = 4 does not fit
  pl.wc = (t.no_window || p > 3 || !t.wk) ? 0 : t.win_chunks;
  const bool win = pl.recur && pl.wc > 0;  // (recurrence form only: the unpreconditioned solve)
  // 16-bit words: the default of a context (st_hess_traits; MI355OPT_WORDS16=0 keeps the 4-byte words) wherever the
  // matrix has them, its far columns are computed and none of them is a halo column.  On cfg2 they shorten the pass by
  // halving the matrix stream (28 -> 16 MB of 128 MB) at the same bits (profiles/words16_default_ab.md).
  const bool w16 = pl.fard && !t.halo && t.wk16 && t.words16;
  pl.form = win ? ST_HESS_WINDOW : ST_HESS_PLAIN, pl.block = win ? kWinBlock : kBlock;
  pl.run_table = win && !t.uniform_grid;  // planned runs of whole tiles (sparse.hip window_bounds)
  pl.twok = gram_count == -2;  // the two-kernel step (opt-in experiment): stpcg.hip asks for it only where twok says it exists
  if (pl.twok && !(win && pl.fard && !t.halo && !w16 && p == 3 && t.twok_r))
    return fail("internal: two-kernel step without its Hessian form");
  // window form: far columns loaded / computed (some of them halo columns of a row shard) / computed with 16-bit words
  if (win) pl.pk = true, pl.hw = hw, pl.far = w16 ? 2 : pl.fard ? 1 : 0;
  else pl.pk = t.pk, pl.from_slots = t.slot_mode && !pl.recur;
  return MI_OK;
}
// mi_dirgram::twok: apply_dir(gram_count = -2) exists -- p = 3, window form with computed far columns, one rank
bool st_hess_twok_exists(int p, StHessTraits t) {
  StHessPlan pl;
  t.twok_r = true;
  return !t.uniform_grid && st_hess_plan(p, -2, t, &pl) == MI_OK && pl.twok;
}

// The instantiations of the three kernel templates that exist: exactly those a plan can name.
template <int P, bool F, bool HL, bool RC, bool PK, int HW, int FAR, bool TWOK>
const void *st_fused_fn() {
  constexpr bool plain = HW == 0 && FAR == 0 && !TWOK && !(RC && F);
  constexpr bool window = HW > 0 && !F && RC && PK && !(FAR == 2 && HL) && (!TWOK || (P == 3 && FAR == 1 && !HL));
  if constexpr (plain || window) return (const void *)k_st_hess_fused<P, F, HL, RC, PK, HW, FAR, TWOK>;
  else return nullptr;
}
template <int P, int HW, bool FARD>
const void *st_widewin_fn() {
  if constexpr (P >= 4 && HW > 0) return (const void *)k_st_hess_widewin<P, HW, FARD>;
  else return nullptr;
}
template <int P, bool HL, bool PK, bool QUAD>
const void *st_wide_fn() {
  if constexpr (P < 5) return nullptr;
  else if constexpr (QUAD) return (const void *)k_st_hess_wideq<P, HL, PK>;
  else return (const void *)k_st_hess_wide<P, HL, PK>;
}
// entries per slice of a window kernel (0: none) and its far-column form
#define DISPATCH_HW(hw, ...) DISPATCH_3(hw, HW, 0, 7, 8, __VA_ARGS__)
#define DISPATCH_FAR(far, ...) DISPATCH_3(far, FAR, 0, 1, 2, __VA_ARGS__)
int st_hess_kernel(int p, const StHessPlan &pl, const void **fn) {
  *fn = nullptr;
  if (pl.form == ST_HESS_WIDEWIN) {
    DISPATCH_P(p, DISPATCH_HW(pl.hw, DISPATCH_FLAG(pl.far != 0, FARD, *fn = st_widewin_fn<P, HW, FARD>())));
  } else if (pl.form == ST_HESS_WIDE || pl.form == ST_HESS_WIDEQ) {
    DISPATCH_P(p, DISPATCH_FLAG(pl.halo, HL, DISPATCH_FLAG(pl.pk, PK, DISPATCH_FLAG(pl.form == ST_HESS_WIDEQ, QUAD,
                                                                                   *fn = st_wide_fn<P, HL, PK, QUAD>()))));
  } else {
    DISPATCH_P4(p, DISPATCH_HW(pl.hw, DISPATCH_FAR(pl.far, DISPATCH_FLAG(pl.from_slots, F, DISPATCH_FLAG(pl.halo, HL,
        DISPATCH_FLAG(pl.recur, RC, DISPATCH_FLAG(pl.pk, PK, DISPATCH_FLAG(pl.twok, TWOK,
            *fn = st_fused_fn<P, F, HL, RC, PK, HW, FAR, TWOK>()))))))));
  }
  if (!*fn) {
    set_error("internal: the one-pass Hessian has no kernel of form %d for p = %d", pl.form, p);
    return MI_ERR_INTERNAL;
  }
  return MI_OK;
}

// resident workgroups per CU of the window instantiation that will run (registers + LDS), asked of the runtime once
// per instantiation and context: the launch plan must fit one round.  (The 16-bit-word and two-kernel variants are
// planned with the answer for their base form, FAR = 1.)
int window_occupancy(mi_ctx *ctx, int p, StHessPlan pl) {
  int &slot = ctx->st_win_occ[p][pl.halo ? 1 : 0][pl.hw == 7 ? 0 : 1][pl.fard ? 1 : 0];
  if (slot == 0) {
    pl.far = pl.fard ? 1 : 0, pl.twok = false;
    const void *fn = nullptr;
    int nb = 0;
    const bool ok = st_hess_kernel(p, pl, &fn) == MI_OK &&
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kWinBlock, 0) == hipSuccess;
    slot = (ok && nb > 0) ? nb : 1;
    (void)hipGetLastError();
  }
  return slot;
}

int rq_apply_dir(mi_op *self, const mi_vec *in, mi_vec *out, int gram_count, int *nparts) {
  mi_stiefel_rq *q = (mi_stiefel_rq *)self->impl;
  mi_ctx *ctx = q->ctx;
  const mi_csr *A = q->A;
  const int p = q->p;
  StHessPlan pl;
  if (const int st = st_hess_plan(p, gram_count, st_hess_traits(ctx, A), &pl)) {
    set_error("%s", pl.error);
    return st;
  }
  const void *fn = nullptr;
  MI_TRY(st_hess_kernel(p, pl, &fn));
  const bool capped = ctx->max_grid < kMaxGrid;  // (lowered explicitly: MI355OPT_MAX_GRID)
  const int ntiles = (int)((A->nslices + kWinWaves - 1) / kWinWaves);
  int grid = 0;
  const int *bounds = nullptr;
  if (pl.form == ST_HESS_WIDEWIN) {
    bool &attr_set = ctx->st_widewin_lds[p - 4][pl.hw == 7 ? 0 : 1][pl.far];
    if (!attr_set) {  // (more than 64 KB of dynamic LDS needs the attribute)
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - 8 * 1024));
      if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("k_st_hess_widewin<%d, %d, %s>: the dynamic LDS limit cannot be raised: %s", p, pl.hw,
                  pl.far ? "true" : "false", hipGetErrorString(e));
        return MI_ERR_HIP;
      }
      attr_set = true;
    }
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kWinBlock, pl.lds_bytes) != hipSuccess || occ < 1) occ = 1;
    (void)hipGetLastError();
    int wgs = std::min(std::min(occ, 2) * ctx->num_cu, kMaxRows);  // (p >= 4: at most two workgroups per CU)
    if (capped) wgs = std::min(wgs, ctx->max_grid);
    MI_TRY(window_bounds(ctx, A, wgs, ntiles, &grid, &bounds));
  } else if (pl.form == ST_HESS_WIDE || pl.form == ST_HESS_WIDEQ) {
    // 256-thread workgroups, as many per CU as the kernel is held to (kWideWavesPerSimd: one wave per SIMD each): one resident
    // round, at most kMaxRows partial rows; several ranks in rows mode need exactly kMaxGrid of them
    const size_t wgs = (A->nslices + kWideWaves - 1) / kWideWaves;
    const int resident = ctx->num_cu * kWideWavesPerSimd;
    grid = ctx->uniform_grid ? kMaxGrid : (int)std::max<size_t>(1, std::min<size_t>(wgs, std::min(resident, kMaxRows)));
    if (!ctx->uniform_grid && capped) grid = std::min(grid, ctx->max_grid);
    if (pl.run_table) MI_TRY(window_bounds(ctx, A, grid, (int)wgs, &grid, &bounds));
  } else {
    // one workgroup per CU and one round (the kernel needs > 64 VGPRs: a second round would only repeat the
    // prologue); the rows mode of several ranks needs the uniform 512-row partial layout instead
    constexpr int cap = 256;
    grid = uniform_grid(ctx, sell_groups(A));
    if (!ctx->uniform_grid && grid > cap) grid = cap;
    if (pl.run_table) {
      // the workgroup budget: what is resident at once (one round), at most kMaxRows partial rows
      const int occ = std::min(window_occupancy(ctx, p, pl), kWaves / kWinWaves);
      int wgs = std::min(cap * occ, kMaxRows);
      // (one-GPU rehearsals of several ranks: the pass waits for its neighbours in its prologue, so -- like the CG
      // kernels -- it must leave room for their kernels while it does; mi_internal.h mi_ctx::max_grid)
      if (capped) wgs = std::min(wgs, ctx->max_grid);
      MI_TRY(window_bounds(ctx, A, wgs, ntiles, &grid, &bounds));
    }
  }
  HaloWaitArg<true> hw_halo;  // a push folded into the kernel that wrote `in`: the pass waits in its prologue
  HaloWaitArg<false> hw_none;
  if (pl.exchange) MI_TRY(comm_halo_exchange_or_wait(ctx, A, p, in->d, &hw_halo.w));
  hw_halo.halo_lo = (unsigned)A->halo_lo;  // (computed far columns of a row shard: spmm_core.h load_far)
  hw_halo.halo_hi = (unsigned)A->halo_hi;
  SellView view = sell_view(A);  // after the exchange: it selects the halo buffer the rows landed in
  const double *slots = ctx->scalars + SLOT_GRAM;
  if (pl.gram_reduce) {
    if (rows_mode(ctx)) MI_TRY(comm_allreduce_rows(ctx, ctx->partials2, nsym(p)));
    if (pl.from_slots) MI_TRY(sharded_reduce(ctx, gram_count, nsym(p), ctx->scalars + SLOT_GRAM));
  }
  const bool fused = pl.form == ST_HESS_PLAIN || pl.form == ST_HESS_WINDOW;
  WinView wv{A->wk, A->wfar, pl.wc, 2 * kWinWaves + 2 * pl.wc, A->win_zero, bounds,
             pl.fard ? (unsigned)A->win_far_pure : 0u, fused ? A->wk16 : nullptr};
  const CgState *live = ctx->cg_live;
  const double *V = in->d, *X = q->X->d, *Y = q->Y->d, *S = q->S_dev, *gram = ctx->partials2,
               *gdir = ctx->scalars + SLOT_GDIR, *rres = pl.twok ? ctx->twok_r : nullptr;
  double *outp = out->d, *parts = ctx->partials;
  void *hwait = pl.halo ? (void *)&hw_halo : (void *)&hw_none;
  // the three kernel signatures
  void *a_fused[] = {&view, &wv, &live, &V, &X, &Y, &S, &gram, &gram_count, &slots, &gdir, &outp, &parts, hwait, &rres};
  void *a_widewin[] = {&view, &wv, &live, &V, &X, &Y, &S, &gdir, &outp, &parts};
  void *a_wide[] = {&view, &live, &V, &X, &Y, &S, &gdir, &outp, &parts, hwait, &bounds};
  void **args = fused ? a_fused : pl.form == ST_HESS_WIDEWIN ? a_widewin : a_wide;
  KScope ks(ctx, MI_K_STIEFEL_HESS_FUSED);
  MI_HIP(hipLaunchKernel(fn, dim3(grid), dim3(pl.block), args, pl.lds_bytes, ctx->stream));
  *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// rows of 9 ... 16 doubles: the objective .5 tr(sym(X'AX)) from the reduced 16 x 16 Gram row (tall_reduce) as read back
double tall_half_trace(const double *G, int p) {
  double tr = 0;
  for (int a = 0; a < p; ++a) tr += G[a * 16 + a];
  return .5 * tr;
}
// ... that row (kTallTile doubles) and, if k > 0, slots [SLOT_MISC, SLOT_MISC + k) behind ONE host synchronisation
int read_tall_row(mi_ctx *ctx, double *G, int k, double *misc) {
  const void *dev[2] = {tall_reduced_row(ctx), ctx->scalars + SLOT_MISC};
  const size_t bytes[2] = {kTallTile * sizeof(double), (size_t)k * sizeof(double)};
  void *host[2] = {G, misc};
  return readback_sync(ctx, k > 0 ? 2 : 1, dev, bytes, host);
}
// The objective .5 tr(sym(X'AX)) of the Gram rows just reduced and, behind the same single host synchronisation, the
// k <= 4 slots [SLOT_MISC, SLOT_MISC + k).  Narrow rows: the packed symmetric Gram sits in the slots from SLOT_GRAM
// (reduce_rows_allreduce) and ONE contiguous range is read, up to the last slot asked for; rows of 9 ... 16 doubles: 136
// packed entries do not fit those slots, the reduced row (tall_reduce) is read back itself.
int read_objective(mi_ctx *ctx, int p, double *f, int k, double *misc) {
  if (tall_p(p)) {
    double Gt[kTallTile];
    MI_TRY(read_tall_row(ctx, Gt, k, misc));
    *f = tall_half_trace(Gt, p);
    return MI_OK;
  }
  static_assert(SLOT_GRAM < SLOT_MISC && SLOT_MISC + 4 <= kScalarSlots, "slot map");
  double buf[SLOT_MISC + 4 - SLOT_GRAM];
  MI_TRY(read_slots_sync(ctx, SLOT_GRAM, k > 0 ? SLOT_MISC + k - SLOT_GRAM : nsym(p), buf));
  double tr = 0;
  for (int a = 0, idx = 0; a < p; ++a) {  // diagonal entries of the packed symmetric Gram
    tr += buf[idx];
    idx += p - a;
  }
  *f = .5 * tr;
  for (int i = 0; i < k; ++i) misc[i] = buf[SLOT_MISC - SLOT_GRAM + i];
  return MI_OK;
}

// What mi_stiefel_rq_trial and mi_stiefel_rq_armijo_trial do once the trial point exists: A X+ with the Gram rows of
// sym(X+'A X+) -- the objective, reduced exactly as mi_stiefel_rq_objective does, and through the same rows S+ and the
// gradient at X+, exactly as mi_stiefel_rq_model does -- then |grad f(X+)|^2 into slot SLOT_MISC + k - 1 and the ONE
// read-back: out[0] = f(X+), out[1 ... k] = slots [SLOT_MISC, SLOT_MISC + k).  Leaves q->trial set to X+.
int rq_trial_chain(mi_stiefel_rq *q, const mi_vec *X_trial, int k, double *out) {
  mi_ctx *ctx = q->ctx;
  const size_t N = q->n * (size_t)q->p;
  if (!q->Y_next) {
    MI_TRY(mi_vec_create(ctx, N, &q->Y_next));
    MI_TRY(mi_vec_create(ctx, N, &q->grad_next));
    MI_HIP(hipMalloc((void **)&q->S_next, kMaxPTall * kMaxPTall * sizeof(double)));
  }
  int count = 0;
  MI_TRY(launch_spmm_gram(ctx, q->A, q->p, nullptr, X_trial->d, X_trial->d, nullptr, q->Y_next->d, &count));
  const bool tall = tall_p(q->p);
  // (rows of 9 ... 16 doubles: the Gram rows are reduced once, into the row the finish pass and the read-back share)
  if (tall) MI_TRY(tall_reduce(ctx, count));
  else MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, count, nsym(q->p), ctx->scalars + SLOT_GRAM));
  MI_TRY(launch_finish(ctx, q->n, q->p, nullptr, X_trial->d, q->Y_next->d, nullptr, tall ? 0 : count, q->S_next,
                       q->grad_next->d, false, nullptr));
  const double *gn[1] = {q->grad_next->d};
  MI_TRY(dot_batch_to_slots(ctx, 1, gn, gn, N, SLOT_MISC + k - 1));
  MI_TRY(read_objective(ctx, q->p, &out[0], k, out + 1));
  q->trial.set(X_trial);
  return MI_OK;
}

struct RqPreconImpl {
  mi_stiefel_rq *q;
  const mi_vec *X;
  const mi_vec *dinv;
};
int rq_precon_apply(mi_precon *self, const mi_vec *r, mi_vec *v) {
  RqPreconImpl *im = (RqPreconImpl *)self->impl;
  mi_stiefel_rq *q = im->q;
  mi_ctx *ctx = q->ctx;
  const int p = q->p;
  if (tall_p(p)) {
    int count = 0;
    MI_TRY(tall_gram(ctx, q->n, p, 2, true, im->X->d, r->d, im->dinv->d, q->Z->d, &count));
    return launch_finish(ctx, q->n, p, nullptr, im->X->d, q->Z->d, nullptr, count, nullptr, v->d, false, nullptr);
  }
  const int grid = row_grid(q->ctx, q->n, p);
  DISPATCH_P(p, hipLaunchKernelGGL((k_st_gram<P, 2, true>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, q->n,
                                   (const double *)im->X->d, (const double *)r->d,
                                   (const double *)im->dinv->d, q->Z->d, ctx->partials2));
  return launch_finish(ctx, q->n, q->p, nullptr, im->X->d, q->Z->d, nullptr, grid, nullptr, v->d, false,
                       nullptr);
}
void rq_precon_destroy(mi_precon *self) { delete (RqPreconImpl *)self->impl; }

}  // namespace

extern "C" {

#ifdef MI_WIN_STAMPS
// experiment builds: (de)register the device buffer the window kernel dumps its stamps into
__attribute__((visibility("default"))) int mi_debug_stamp_buffer(void *dev_ptr) {
  MI_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mi::g_stamp_buf), &dev_ptr, sizeof(dev_ptr)));
  return MI_OK;
}
#endif

// Host-only: the launch plan of the one-pass Hessian (st_hess_plan) for plain numbers -- see include/mi355opt.h
static int hess_form_numbers(int p, int gram_count, const StHessTraits &t, int out[14]) {
  StHessPlan pl;
  const int st = st_hess_plan(p, gram_count, t, &pl);
  if (st != MI_OK) set_error("%s", pl.error);
  const int v[14] = {pl.form, pl.from_slots, pl.halo, pl.recur, pl.pk, pl.hw, pl.far, pl.twok, pl.block, (int)pl.lds_bytes,
                     pl.run_table, pl.exchange, pl.gram_reduce, st_hess_twok_exists(p, t)};
  std::copy(v, v + 14, out);
  return st;
}
int mi_debug_stiefel_hess_form(int p, int gram_count, const size_t m[9], const int s[9], int out[14]) {
  MI_REQUIRE(m && s && out, "null argument");
  const StHessTraits t{m[0] != 0, m[1] != 0, m[2] != 0, (int)m[3], (int)m[4], m[5], m[6], m[7] != 0, m[8] != 0,
                       s[0] != 0, s[1] != 0, s[2] != 0, s[5] != 0, s[6] != 0, s[7] != 0, s[8] != 0, s[3], s[4]};
  return hess_form_numbers(p, gram_count, t, out);
}
// ... and for a matrix on a context as they stand: the plan mi_stpcg's Hessian pass would be launched by right now
int mi_debug_stiefel_hess_form_of(const mi_ctx *ctx, const mi_csr *A, int p, int gram_count, int out[14]) {
  MI_REQUIRE(ctx && A && out, "null argument");
  return hess_form_numbers(p, gram_count, st_hess_traits(ctx, A), out);
}

int mi_stiefel_gram(mi_ctx *ctx, size_t n, int p, const mi_vec *X, const mi_vec *Z, double *G_host) {
  MI_TRY(check_np(ctx, n, p, X, Z, nullptr));
  MI_REQUIRE(X && Z && G_host, "null argument");
  if (tall_p(p)) {  // raw 16 x 16 rows -> the reduced row -> host
    int count = 0;
    MI_TRY(tall_gram(ctx, n, p, 0, false, X->d, Z->d, nullptr, nullptr, &count));
    MI_TRY(tall_reduce(ctx, count));
    double G[kTallTile];
    MI_TRY(read_tall_row(ctx, G, 0, nullptr));
    for (int a = 0; a < p; ++a)
      for (int b = 0; b < p; ++b) G_host[a * p + b] = G[a * 16 + b];
    return MI_OK;
  }
  const int grid = row_grid(ctx, n, p);
  DISPATCH_P(p, hipLaunchKernelGGL((k_st_gram<P, 0, false>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, n,
                                   (const double *)X->d, (const double *)Z->d, (const double *)nullptr,
                                   (double *)nullptr, ctx->partials2));
  double *slots = ctx->scalars + SLOT_RAW;
  MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, grid, p * p, slots));
  return read_slots_sync(ctx, SLOT_RAW, p * p, G_host);
}

int mi_stiefel_project(mi_ctx *ctx, size_t n, int p, const mi_vec *X, const mi_vec *Z, mi_vec *out) {
  MI_TRY(check_np(ctx, n, p, X, Z, out));
  MI_REQUIRE(X && Z && out, "null argument");
  touch(out);
  if (tall_p(p)) {
    int count = 0;
    MI_TRY(tall_gram(ctx, n, p, 0, true, X->d, Z->d, nullptr, nullptr, &count));
    return launch_finish(ctx, n, p, nullptr, X->d, Z->d, nullptr, count, nullptr, out->d, false, nullptr);
  }
  const int grid = row_grid(ctx, n, p);
  DISPATCH_P(p, hipLaunchKernelGGL((k_st_gram<P, 0, true>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, n,
                                   (const double *)X->d, (const double *)Z->d, (const double *)nullptr,
                                   (double *)nullptr, ctx->partials2));
  return launch_finish(ctx, n, p, nullptr, X->d, Z->d, nullptr, grid, nullptr, out->d, false, nullptr);
}

int mi_stiefel_retract(mi_ctx *ctx, size_t n, int p, const mi_vec *X, const mi_vec *V, mi_vec *Y) {
  MI_TRY(check_np(ctx, n, p, X, V, Y));
  MI_REQUIRE(X && V && Y, "null argument");
  touch(Y);
  const int grid = row_grid(ctx, n, p);
  KScope ks(ctx, MI_K_STIEFEL_RETRACT);
  if (tall_p(p)) {  // Y = X + V with the rows of Y'Y, then the polar factor
    int count = 0;
    MI_TRY(tall_gram(ctx, n, p, 1, true, X->d, V->d, nullptr, Y->d, &count));
    return tall_polar(ctx, n, p, Y->d, count);
  }
  DISPATCH_P(p, hipLaunchKernelGGL((k_st_gram<P, 1, true>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, n,
                                   (const double *)X->d, (const double *)V->d, (const double *)nullptr,
                                   Y->d, ctx->partials2));
  double *slots = ctx->scalars + SLOT_GRAM;
  if (ctx->comm != nullptr || ctx->force_slot_path) {
    MI_TRY(sharded_reduce(ctx, grid, nsym(p), slots));
    DISPATCH_P(p, hipLaunchKernelGGL((k_st_polar<P, true>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, n,
                                     Y->d, (const double *)ctx->partials2, grid, (const double *)slots));
  } else {
    DISPATCH_P(p, hipLaunchKernelGGL((k_st_polar<P, false>), dim3(grid), dim3(StBlk<P>::threads), 0, ctx->stream, n,
                                     Y->d, (const double *)ctx->partials2, grid, (const double *)slots));
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int mi_stiefel_rq_create(mi_ctx *ctx, const mi_csr *A, size_t n, int p, mi_stiefel_rq **out) {
  MI_REQUIRE(ctx && A && out, "null argument");
  MI_REQUIRE(p >= 1 && p <= kMaxPTall, "p must be in [1,%d], got %d", kMaxPTall, p);
  MI_REQUIRE(A->n == n && A->ctx == ctx, "matrix has %zu rows, expected %zu", A->n, n);
  if (tall_p(p)) MI_TRY(tall_check(ctx, A, n, p));
  mi_stiefel_rq *q = new mi_stiefel_rq();
  q->ctx = ctx;
  q->A = A;
  q->n = n;
  q->p = p;
  q->X = nullptr;
  MI_HIP(hipMalloc((void **)&q->S_dev, kMaxPTall * kMaxPTall * sizeof(double)));
  MI_HIP(hipMemsetAsync(q->S_dev, 0, kMaxPTall * kMaxPTall * sizeof(double), ctx->stream));
  MI_TRY(mi_vec_create(ctx, n * (size_t)p, &q->Z));
  MI_TRY(mi_vec_create(ctx, n * (size_t)p, &q->Y));
  q->hess.ctx = ctx;
  q->hess.n = n * (size_t)p;
  q->hess.apply = rq_apply;
  q->hess.apply_dots = rq_apply_dots;
  q->hess.apply_dir = rq_apply_dir;
  q->hess.impl = q;
  q->hess.borrowed = true;
  *out = q;
  return MI_OK;
}

int mi_stiefel_rq_destroy(mi_stiefel_rq *q) {
  if (!q) return MI_OK;
  (void)hipStreamSynchronize(q->ctx->stream);
  (void)hipFree(q->S_dev);
  (void)hipFree(q->S_next);
  mi_vec_destroy(q->Z);
  mi_vec_destroy(q->Y);
  mi_vec_destroy(q->Y_next);
  mi_vec_destroy(q->grad_next);
  mi_vec_destroy(q->Hh);
  delete q;
  return MI_OK;
}

int mi_stiefel_rq_objective(mi_stiefel_rq *q, const mi_vec *X, double *f) {
  MI_REQUIRE(q && X && f, "null argument");
  MI_TRY(check_np(q->ctx, q->n, q->p, X, nullptr, nullptr));
  mi_ctx *ctx = q->ctx;
  q->trial.clear();  // (Z is scratch of both)
  int count = 0;
  MI_TRY(launch_spmm_gram(ctx, q->A, q->p, nullptr, X->d, X->d, nullptr, q->Z->d, &count));
  if (tall_p(q->p)) MI_TRY(tall_reduce(ctx, count));
  else MI_TRY(reduce_rows_allreduce(ctx, ctx->partials2, count, nsym(q->p), ctx->scalars + SLOT_GRAM));
  return read_objective(ctx, q->p, f, 0, nullptr);
}

int mi_stiefel_rq_model(mi_stiefel_rq *q, const mi_vec *X, mi_vec *grad, mi_op **hess) {
  MI_REQUIRE(q && X && grad, "null argument");
  MI_TRY(check_np(q->ctx, q->n, q->p, X, grad, nullptr));
  int count = 0;
  touch(grad);
  if (q->trial.is(X)) {
    // X is the point mi_stiefel_rq_trial just evaluated: A X, S and the gradient exist already
    std::swap(q->Y, q->Y_next);
    std::swap(q->S_dev, q->S_next);
    MI_TRY(mi_vec_copy(grad, q->grad_next));
  } else {
    // Y = A X (kept: the direction-Gram identity needs it) ; S = sym(X'AX) (kept on the device for the
    // Hessian) ; grad = Y - X S
    MI_TRY(launch_spmm_gram(q->ctx, q->A, q->p, nullptr, X->d, X->d, nullptr, q->Y->d, &count));
    MI_TRY(launch_finish(q->ctx, q->n, q->p, nullptr, X->d, q->Y->d, nullptr, count, q->S_dev, grad->d, false,
                         nullptr));
  }
  q->trial.clear();
  q->X = X;
  q->X_serial = X->serial;
  q->dg.p = q->p;
  q->dg.n = q->n;
  q->dg.X = X->d;
  q->dg.Y = q->Y->d;
  q->dg.S = q->S_dev;
  q->dg.halo_A = q->A->halo ? q->A : nullptr;
  // (the opt-in two-kernel step: p = 3, window form with computed far columns, one rank.  Asked for a context that HAS
  // opted in: the switch may be set on this context after the model exists, and mi_stpcg reads it per solve)
  q->dg.twok = st_hess_twok_exists(q->p, st_hess_traits(q->ctx, q->A, true));
  // the one-pass kernel uses 32-bit byte offsets: fields of 4 GiB or more keep the two-pass operator -- and so does
  // a matrix that is not symmetric (checked at creation): the one-pass form replaces X'(A p) by (A X)'p
  // rows of 9 ... 16 doubles have no one-pass form (st_hess_plan): STPCG drives the two-pass operator through
  // apply_dots, the three curvature dots fused into its last pass
  q->hess.dirgram = (sell_stream_ok(q->A, q->p) && q->A->symmetric && !tall_p(q->p)) ? &q->dg : nullptr;
  if (!q->A->symmetric && !q->warned_unsymmetric) {
    q->warned_unsymmetric = true;
    fprintf(stderr, "mi355opt: the matrix of this Stiefel Rayleigh-quotient problem is not symmetric: the Hessian "
                    "operator keeps its two-pass form (P_X(A V - V S) with A as given)\n");
  }
  if (hess) *hess = &q->hess;
  return MI_OK;
}

// One trial step of a trust-region / line-search method at the point X the model is bound to (reference
// Riemannian/TNT.h:493-512,573-585): step norm, retraction, objective at the trial point, predicted-decrease terms and
// -- speculatively -- the model at the trial point, as ONE launch chain and ONE read-back.  Every number is produced
// by the same kernels, in the same order of summation, as the separate calls (mi_vec_dot_batch, mi_stiefel_retract,
// mi_stiefel_rq_objective, mi_stiefel_rq_model) would: only one sparse product (A X+ serves the objective AND the
// next gradient) and the intermediate synchronisations disappear.
//   out[0] = f(X+), out[1] = <h,h>, out[2] = <g,h>, out[3] = <h, Hess h>, out[4] = |grad f(X+)|^2
int mi_stiefel_rq_trial(mi_stiefel_rq *q, const mi_vec *X, const mi_vec *h, const mi_vec *g, mi_vec *X_trial,
                        double out[5]) {
  MI_REQUIRE(q && X && h && g && X_trial && out, "null argument");
  MI_REQUIRE(bound_to(q->X, q->X_serial, X),
             "mi_stiefel_rq_trial: the model is not bound to this X (call mi_stiefel_rq_model first)");
  MI_TRY(check_np(q->ctx, q->n, q->p, X, h, g));
  MI_TRY(check_np(q->ctx, q->n, q->p, X_trial, nullptr, nullptr));
  mi_ctx *ctx = q->ctx;
  ctx->fusion.fused_trial_steps++;
  const size_t N = q->n * (size_t)q->p;
  if (!q->Hh) MI_TRY(mi_vec_create(ctx, N, &q->Hh));
  q->trial.clear();
  // (a) Hess h, then |h|^2, <g,h>, <h, Hess h> in one pass (as MI355::dot_batch does)
  MI_TRY(rq_apply(&q->hess, h, q->Hh));
  {
    const double *xs[3] = {h->d, g->d, h->d}, *ys[3] = {h->d, h->d, q->Hh->d};
    MI_TRY(dot_batch_to_slots(ctx, 3, xs, ys, N, SLOT_MISC));
  }
  // (b) X+ = polar(X + h)
  MI_TRY(mi_stiefel_retract(ctx, q->n, q->p, X, h, X_trial));
  // (c) f(X+), the model at X+ and |grad f(X+)|^2 behind the three dots; (d) one read-back
  return rq_trial_chain(q, X_trial, 4, out);
}

// One Armijo trial of a backtracking line search along -g (reference Riemannian/GradientDescent.h:266-286:
// h = -t g; x_trial = retract(x, h); f(x_trial)) plus, speculatively, the gradient at the trial point and its squared
// norm (:325-327, used if the trial is accepted): one launch chain, one read-back.  Same kernels and summation
// orders as the separate calls.  out[0] = f(X+), out[1] = |grad f(X+)|^2.
int mi_stiefel_rq_armijo_trial(mi_stiefel_rq *q, const mi_vec *X, const mi_vec *g, double t, mi_vec *h_out,
                               mi_vec *X_trial, double out[2]) {
  MI_REQUIRE(q && X && g && h_out && X_trial && out, "null argument");
  MI_REQUIRE(bound_to(q->X, q->X_serial, X),
             "mi_stiefel_rq_armijo_trial: the model is not bound to this X (call mi_stiefel_rq_model first)");
  MI_TRY(check_np(q->ctx, q->n, q->p, X, g, h_out));
  MI_TRY(check_np(q->ctx, q->n, q->p, X_trial, nullptr, nullptr));
  mi_ctx *ctx = q->ctx;
  ctx->fusion.fused_trial_steps++;
  q->trial.clear();
  touch(X_trial);
  MI_TRY(mi_vec_scale_to(h_out, -t, g));  // h = -t * g (:276)
  MI_TRY(mi_stiefel_retract(ctx, q->n, q->p, X, h_out, X_trial));
  return rq_trial_chain(q, X_trial, 1, out);
}

int mi_stiefel_rq_precon(mi_stiefel_rq *q, const mi_vec *X, const mi_vec *dinv_rows, mi_precon **out) {
  MI_REQUIRE(q && X && dinv_rows && out, "null argument");
  MI_TRY(check_np(q->ctx, q->n, q->p, X, nullptr, nullptr));
  MI_REQUIRE(dinv_rows->n == q->n, "dinv_rows must have one entry per row");
  mi_precon *P = new mi_precon();
  P->ctx = q->ctx;
  P->n = q->n * (size_t)q->p;
  P->kind = 0;
  P->apply = rq_precon_apply;
  P->destroy = rq_precon_destroy;
  P->impl = new RqPreconImpl{q, X, dinv_rows};
  *out = P;
  return MI_OK;
}

}  // extern "C"
