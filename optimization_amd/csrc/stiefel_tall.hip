// stiefel_tall.hip -- the "tall rows" kernel family: Stiefel St(n,p) for rows of 9 ... 16 doubles (p a run-time
// argument), the third family next to the per-thread-matrix kernels (p <= 4) and the LDS-matrix kernels (p = 5 ... 8)
// of stiefel.hip.  Those keep P x P accumulators per thread and one matrix entry per lane of a wave; at P = 16 that is
// 256 doubles per thread.  Here a wave owns a TILE of 16 rows x 16 columns laid out as the fp64 matrix pipe wants it:
//     lane l  <->  column l & 15, rows (l >> 4) + 4 j, j = 0 ... 3     (4 doubles per lane)
// which is the C / D layout of v_mfma_f64_16x16x4_f64 (A operand A[l & 15][l >> 4], B operand B[l >> 4][l & 15]), so
//   * G += X'Z: the four rows 4 j ... 4 j + 3 of a tile of X and of Z ARE the A and B operands of one MFMA -- no
//     shuffle, no LDS transpose;
//   * out = Z - X M: lane l loads X[row l & 15][4 (l >> 4) + k] and holds M[4 (l >> 4) + k][l & 15], k = 0 ... 3: the
//     operands of four MFMAs whose result lands in the tile layout of Z (the sum over the sixteen values of the
//     contraction index is only taken in another order: k inside, l >> 4 outside);
//   * the sparse product accumulates in the tile layout: the sixteen lanes of a row gather one row of V (72 ... 128
//     contiguous bytes) per entry, products and sums rounded separately in storage order as in spmm_core.h.
// Columns >= p carry zeros.  No atomics; every reduction has a fixed shape.
// Gram partial rows: the whole 16 x 16 tile per workgroup, row-major in ctx->partials2 (stiefel_tall.h) -- at most
// kTallRows = 255 workgroups leave one, row 255 is the sum a one-workgroup reduce kernel leaves (tall_reduce).
#include "stiefel_tall.h"
#include "spmm_core.h"

#include <algorithm>

using namespace mi;

namespace {

constexpr int kTallBlock = kBlock, kTallWaves = kWaves;  // 1024 threads: 16 tiles of 16 rows per workgroup step
typedef double tile4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ tile4 mma(double a, double b, tile4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// thread t < kTallTile: entry t of the sum of `count` Gram rows, rows in order (the reduce kernel and a consumer's
// prologue run this very loop: same bits either way); entries outside p x p are zero
__device__ __forceinline__ double tall_row_sum(const double *__restrict__ rows, int count, int p, int t) {
  double s = 0;
  if ((t >> 4) < p && (t & 15) < p) {
    int r = 0;
    for (; r + 8 <= count; r += 8) {
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = rows[(size_t)(r + i) * kTallTile + t];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; r < count; ++r) s += rows[(size_t)r * kTallTile + t];
  }
  return s;
}

// the waves' Gram tiles -> this workgroup's partial row (SYM: symmetrised).  lds: kTallWaves * kTallTile doubles
template <bool SYM>
__device__ __forceinline__ void tall_store_gram(const tile4 &G, double *lds, double *__restrict__ partials) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) lds[((g + 4 * j) * 16 + c) * kTallWaves + w] = G[j];
  __syncthreads();
  if (threadIdx.x < kTallTile) {
    const int t = threadIdx.x, a = t >> 4, b = t & 15;
    double v = sum16(lds + t * kTallWaves);
    if (SYM) v = .5 * (v + sum16(lds + (b * 16 + a) * kTallWaves));
    partials[(size_t)blockIdx.x * kTallTile + t] = v;
  }
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (hi, lo) += a b with the product and the sum exact (fma residual, two-sum); lo collects the errors unnormalised
__device__ __forceinline__ void dd_fma(double a, double b, double &hi, double &lo) {
#pragma clang fp contract(off)
  const double pr = a * b, pe = __builtin_fma(a, b, -pr);
  const double s = hi + pr, bb = s - hi, se = (hi - (s - bb)) + (pr - bb);
  hi = s;
  lo = lo + (se + pe);
}

// G^-1/2 of the p x p SPD matrix G (16 doubles a row) by ONE wave: the scaled coupled Newton-Schulz iteration of
// stiefel.hip dev_sym_invsqrt_wave -- Y0 = G / |G|_F, Z0 = I; T = Z Y; Y <- Y (3 I - T) / 2, Z <- (3 I - T) Z / 2 -- with
// the same stopping rule, four entries per lane instead of one, and one corrective step on the unscaled G behind it.
// work: 3 * kTallTile doubles of LDS; out: kTallTile, zero outside p x p.
__device__ void tall_invsqrt_wave(const double *G, int p, double *work, double *out) {
  double *T = work, *Y = work + kTallTile, *Z = work + 2 * kTallTile;
  const int l = threadIdx.x & 63;
  double s2 = 0;
  for (int i = 0; i < p; ++i)
    for (int j = 0; j < p; ++j) s2 += G[i * 16 + j] * G[i * 16 + j];
  const double sc = sqrt(s2);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = l + 64 * q, i = e >> 4, j = e & 15;
    const bool in = i < p && j < p;
    Y[e] = in ? G[e] / sc : 0.0;
    Z[e] = (in && i == j) ? 1.0 : 0.0;
    T[e] = 0.0;
  }
  wave_sync_lds();
  bool last = false;
  for (int it = 0; it < 100; ++it) {
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = l + 64 * q, i = e >> 4, j = e & 15;
      t[q] = 0;
      for (int k = 0; k < p; ++k) t[q] += Z[i * 16 + k] * Y[k * 16 + j];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) T[l + 64 * q] = t[q];  // (zero outside p x p: Y and Z are)
    wave_sync_lds();
    double err = 0;  // |Z Y - I|_F^2, the same number in every lane
    for (int i = 0; i < p; ++i)
      for (int j = 0; j < p; ++j) {
        const double d = T[i * 16 + j] - (i == j ? 1.0 : 0.0);
        err += d * d;
      }
    double yn[4], zn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = l + 64 * q, i = e >> 4, j = e & 15;
      yn[q] = 0, zn[q] = 0;
      for (int k = 0; k < p; ++k) {
        const double rkj = ((k == j) ? 3.0 : 0.0) - T[k * 16 + j], rik = ((i == k) ? 3.0 : 0.0) - T[i * 16 + k];
        yn[q] += Y[i * 16 + k] * rkj;
        zn[q] += rik * Z[k * 16 + j];
      }
    }
    wave_sync_lds();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = l + 64 * q, i = e >> 4, j = e & 15;
      if (i < p && j < p) {
        Y[e] = .5 * yn[q];
        Z[e] = .5 * zn[q];
      }
    }
    wave_sync_lds();
    if (last) break;
    if (!(err > 1e-26)) last = true;  // (converged to ~1e-13: one more quadratic step finishes it; NaN ends it too)
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = l + 64 * q;
    out[e] = ((e >> 4) < p && (e & 15) < p) ? Z[e] / sqrt(sc) : 0.0;
  }
  wave_sync_lds();
  // One corrective step M <- M + M (I - M G M) / 2 on the UNSCALED G.  At cond(G) = 1e6 a float64 M G M carries a
  // rounding of eps |M| |G| |M| ~ 1e-10, as large as the residual itself, so the two products are accumulated in
  // double-double (dd_fma); the update is plain.  It halves the loss of orthonormality of Y M that the iteration's own
  // rounding leaves (tests/test_gpu_stiefel_tall_parity.py, the retractions with cond(Y'Y) up to 1e6).
  // T, Y <- hi, lo of M G
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = l + 64 * q, i = e >> 4, j = e & 15;
    double hi = 0, lo = 0;
    for (int k = 0; k < p; ++k) dd_fma(out[i * 16 + k], G[k * 16 + j], hi, lo);
    T[e] = hi;
    Y[e] = lo;
  }
  wave_sync_lds();
  // Z <- I - (M G) M
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = l + 64 * q, i = e >> 4, j = e & 15;
    double hi = 0, lo = 0;
    for (int k = 0; k < p; ++k) {
      dd_fma(T[i * 16 + k], out[k * 16 + j], hi, lo);
      lo += Y[i * 16 + k] * out[k * 16 + j];
    }
    Z[e] = (i < p && j < p) ? ((i == j ? 1.0 : 0.0) - hi) - lo : 0.0;
  }
  wave_sync_lds();
  double c[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = l + 64 * q, i = e >> 4, j = e & 15;
    c[q] = 0;
    for (int k = 0; k < p; ++k) c[q] += out[i * 16 + k] * Z[k * 16 + j];
  }
  wave_sync_lds();
#pragma unroll
  for (int q = 0; q < 4; ++q) out[l + 64 * q] += .5 * c[q];  // (zero outside p x p: M and the residual are)
  wave_sync_lds();
}

// ---- kernels -------------------------------------------------------------------------------------------------------

// Z = A V - V S (S nullable) in the tile layout; GRAM: this workgroup's partial row of sym(X'Z).
// A workgroup owns a contiguous run of slices; a wave takes quarter slices (16 rows), the four quarters of a slice in
// neighbouring waves.  The matrix words of a row are read by its sixteen lanes from one address.
template <bool PK, bool GRAM>
__global__ __launch_bounds__(kTallBlock) void k_tall_spmm_gram(SellView A, const CgState *__restrict__ st, int p,
                                                               const double *__restrict__ V, const double *__restrict__ X,
                                                               const double *__restrict__ S, double *__restrict__ Z,
                                                               double *__restrict__ partials) {
  __shared__ double lds[GRAM ? kTallWaves * kTallTile : 1];
  __shared__ double vt[PK ? 256 : 1];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wu = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool colok = c < p;
  const int cc = colok ? c : 0;
  if (PK) {
    if (threadIdx.x < 256) vt[threadIdx.x] = A.vtab[threadIdx.x];
    __syncthreads();
  }
  double sb[4];  // B operand of V S: S[4 g + k][c]
#pragma unroll
  for (int k = 0; k < 4; ++k) sb[k] = (S && colok && 4 * g + k < p) ? S[(4 * g + k) * p + c] : 0.0;
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t s0 = (A.nslices * lb) / nb, s1 = (A.nslices * (lb + 1)) / nb;
  const size_t n = A.n;
  tile4 G = {0.0, 0.0, 0.0, 0.0};
  for (size_t u = 4 * s0 + (size_t)wu; u < 4 * s1; u += kTallWaves) {
    const size_t slice = u >> 2;
    const unsigned r0 = 16u * (unsigned)(u & 3);  // first row of the tile inside its slice
    const long long b0 = slice_bound(A.slice_ptr, slice), b1 = slice_bound(A.slice_ptr, slice + 1);
    size_t row[4];
    bool live[4];
    double acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      row[j] = slice * 64 + r0 + (unsigned)(g + 4 * j);
      live[j] = row[j] < n;
      acc[j] = 0;
    }
    for (long long k = b0; k < b1; ++k) {
      double a[4];
      size_t ci[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t e = (size_t)k * 64 + r0 + (unsigned)(g + 4 * j);
        if (PK) {
          const unsigned wd = A.pk[e];
          a[j] = vt[wd & 255u];
          ci[j] = (size_t)((long long)row[j] + (long long)((int)wd >> 8));
        } else {
          a[j] = A.val[e];
          ci[j] = (size_t)A.col[e];
        }
        if (!live[j]) { a[j] = 0.0; ci[j] = 0; }  // (rows past the last one: no entry, a valid address)
      }
      double gv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[j] = V[ci[j] * (size_t)p + cc];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // product and sum rounded separately, entry by entry in storage order (spmm_core.h sell_stream)
#pragma clang fp contract(off)
        const double t = a[j] * gv[j];
        acc[j] = acc[j] + t;
      }
    }
    tile4 D = {0.0, 0.0, 0.0, 0.0};
    if (S) {  // (V S)(tile): A operand V[row c of the tile][4 g + k]
      const size_t rr = slice * 64 + r0 + (unsigned)c;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double va = (rr < n && 4 * g + k < p) ? V[rr * (size_t)p + 4 * g + k] : 0.0;
        D = mma(va, sb[k], D);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = live[j] && colok;
      const double z = ok ? acc[j] - D[j] : 0.0;
      if (ok) Z[row[j] * (size_t)p + c] = z;
      if (GRAM) {
        const double x = ok ? X[row[j] * (size_t)p + c] : 0.0;
        G = mma(x, z, G);
      }
    }
  }
  if (GRAM) tall_store_gram<true>(G, lds, partials);
}

// Gram partial rows of two dense n x p fields (k_st_gram's variants): 0: X'Z; 1: out = X + Z, out'out;
// 2: out = dinv_rows .* Z, X'out.  SYM: symmetrised rows, else raw.  Waves stride over the 16-row tiles.
template <int VARIANT, bool SYM>
__global__ __launch_bounds__(kTallBlock) void k_tall_gram(size_t n, int p, const double *__restrict__ X,
                                                          const double *__restrict__ Zin, const double *__restrict__ dinv,
                                                          double *__restrict__ out, double *__restrict__ partials) {
  __shared__ double lds[kTallWaves * kTallTile];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wu = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool colok = c < p;
  const size_t ntiles = (n + 15) / 16, stride = (size_t)gridDim.x * kTallWaves;
  tile4 G = {0.0, 0.0, 0.0, 0.0};
  for (size_t t = (size_t)blockIdx.x * kTallWaves + (size_t)wu; t < ntiles; t += stride) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t row = t * 16 + (unsigned)(g + 4 * j);
      const bool ok = row < n && colok;
      const size_t at = ok ? row * (size_t)p + c : 0;
      double x = ok ? X[at] : 0.0, z = ok ? Zin[at] : 0.0;
      if (VARIANT == 1) {
        x = x + z;
        z = x;
        if (ok) out[at] = x;
      } else if (VARIANT == 2) {
        z = (ok ? dinv[row] : 0.0) * z;
        if (ok) out[at] = z;
      }
      G = mma(x, z, G);
    }
  }
  tall_store_gram<SYM>(G, lds, partials);
}

// the `count` Gram rows summed into the reduced row (one workgroup)
__global__ __launch_bounds__(kTallTile) void k_tall_reduce(const double *__restrict__ rows, int count, int p,
                                                           double *__restrict__ reduced) {
  reduced[threadIdx.x] = tall_row_sum(rows, count, p, (int)threadIdx.x);
}

// prologue: M = the sum of the Gram rows (re-reduced by every workgroup, or the one reduced row);
// body: out = Z - X M;  DOTS: partial rows of <Vin,out>, <out,out>, <Vin,Vin>;  M_out (nullable): M, p x p
template <bool DOTS>
__global__ __launch_bounds__(kTallBlock) void k_tall_finish(size_t n, int p, const CgState *__restrict__ st,
                                                            const double *__restrict__ X, const double *__restrict__ Z,
                                                            const double *__restrict__ Vin,
                                                            const double *__restrict__ rows, int count,
                                                            double *__restrict__ M_out, double *__restrict__ out,
                                                            double *__restrict__ partials) {
  __shared__ double Mm[kTallTile];
  __shared__ double lds[3 * kTallWaves];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wu = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool colok = c < p;
  if (threadIdx.x < kTallTile) {
    const int t = threadIdx.x;
    const double m = tall_row_sum(rows, count, p, t);
    Mm[t] = m;
    if (M_out && blockIdx.x == 0 && (t >> 4) < p && (t & 15) < p) M_out[(t >> 4) * p + (t & 15)] = m;
  }
  __syncthreads();
  double mb[4];  // B operand: M[4 g + k][c]
#pragma unroll
  for (int k = 0; k < 4; ++k) mb[k] = Mm[(4 * g + k) * 16 + c];
  const size_t ntiles = (n + 15) / 16, stride = (size_t)gridDim.x * kTallWaves;
  double a[3] = {0, 0, 0};
  for (size_t t = (size_t)blockIdx.x * kTallWaves + (size_t)wu; t < ntiles; t += stride) {
    const size_t rr = t * 16 + (unsigned)c;
    tile4 D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double xa = (rr < n && 4 * g + k < p) ? X[rr * (size_t)p + 4 * g + k] : 0.0;
      D = mma(xa, mb[k], D);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t row = t * 16 + (unsigned)(g + 4 * j);
      const bool ok = row < n && colok;
      const size_t at = ok ? row * (size_t)p + c : 0;
      const double o = ok ? Z[at] - D[j] : 0.0;
      if (ok) out[at] = o;
      if (DOTS) {
        const double vi = ok ? Vin[at] : 0.0;
        a[0] += vi * o; a[1] += o * o; a[2] += vi * vi;
      }
    }
  }
  if (DOTS) block_partials_store<3>(a, lds, partials);
}

// retraction finish: Y <- Y (Y'Y)^-1/2, the inverse square root once per workgroup (wave 0)
__global__ __launch_bounds__(kTallBlock) void k_tall_polar(size_t n, int p, double *__restrict__ Y,
                                                           const double *__restrict__ rows, int count) {
  __shared__ double Gm[kTallTile], Minv[kTallTile], work[3 * kTallTile];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wu = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool colok = c < p;
  if (threadIdx.x < kTallTile) Gm[threadIdx.x] = tall_row_sum(rows, count, p, (int)threadIdx.x);
  __syncthreads();
  if (wu == 0) tall_invsqrt_wave(Gm, p, work, Minv);
  __syncthreads();
  double mb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) mb[k] = Minv[(4 * g + k) * 16 + c];
  const size_t ntiles = (n + 15) / 16, stride = (size_t)gridDim.x * kTallWaves;
  for (size_t t = (size_t)blockIdx.x * kTallWaves + (size_t)wu; t < ntiles; t += stride) {
    // (in place: every lane's operand loads of the tile precede the stores -- they depend on all of them -- and a
    // tile belongs to one wave)
    const size_t rr = t * 16 + (unsigned)c;
    tile4 D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double ya = (rr < n && 4 * g + k < p) ? Y[rr * (size_t)p + 4 * g + k] : 0.0;
      D = mma(ya, mb[k], D);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t row = t * 16 + (unsigned)(g + 4 * j);
      if (row < n && colok) Y[row * (size_t)p + c] = D[j];
    }
  }
}

inline int row_grid_tall(const mi_ctx *ctx, size_t n) { return tall_grid(ctx, (n + 16 * kTallWaves - 1) / (16 * kTallWaves)); }

// the rows a consumer sums in its prologue: the producer's rows themselves (MI355OPT_TALL_PROLOGUE=1), or -- the
// default -- the one row of the reduce kernel
int consumer_rows(mi_ctx *ctx, int count, const double **rows, int *nrows) {
  if (count > 0 && ctx->cfg.tall_prologue) {
    *rows = ctx->partials2;
    *nrows = count;
    return MI_OK;
  }
  if (count > 0) MI_TRY(tall_reduce(ctx, count));
  *rows = tall_reduced_row(ctx);
  *nrows = 1;
  return MI_OK;
}

}  // namespace

namespace mi {

int tall_check(const mi_ctx *ctx, const mi_csr *A, size_t n, int p) {
  MI_REQUIRE(tall_p(p), "internal: the tall-row kernels take rows of %d ... %d doubles, got %d", kMaxP + 1, kMaxPTall, p);
  MI_REQUIRE(ctx->comm == nullptr && !ctx->force_slot_path && !ctx->uniform_grid && !(A && (A->halo || csr_row_sharded(A))),
             "rows of %d ... %d doubles run on one context (no communicator, no row-sharded matrix, no "
             "MI355OPT_FORCE_SLOT_PATH); rows of up to %d doubles run everywhere: got p = %d",
             kMaxP + 1, kMaxPTall, kMaxP, p);
  const size_t lim = (size_t)1 << 32;
  MI_REQUIRE((n + 64) * (size_t)p * 8 < lim && (!A || sell_stream_ok(A, p)), "Stiefel rows of %d doubles need fields below 4 GiB", p);
  return MI_OK;
}

int tall_spmm(mi_ctx *ctx, const mi_csr *A, int p, const double *V, double *W) {
  if (A->n == 0) return MI_OK;
  const int grid = tall_grid(ctx, (A->nslices + 3) / 4);
  SellView view = sell_view(A);
  KScope ks(ctx, MI_K_SPMM);
  DISPATCH_FLAG(A->pk != nullptr, PK,
                hipLaunchKernelGGL((k_tall_spmm_gram<PK, false>), dim3(grid), dim3(kTallBlock), 0, ctx->stream, view,
                                   (const CgState *)nullptr, p, V, (const double *)nullptr, (const double *)nullptr, W,
                                   (double *)nullptr));
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int tall_spmm_gram(mi_ctx *ctx, const mi_csr *A, int p, const CgState *st, const double *V, const double *X,
                   const double *S, double *Z, int *count) {
  const int grid = tall_grid(ctx, (A->nslices + 3) / 4);
  SellView view = sell_view(A);
  KScope ks(ctx, MI_K_STIEFEL_SPMM_GRAM);
  DISPATCH_FLAG(A->pk != nullptr, PK,
                hipLaunchKernelGGL((k_tall_spmm_gram<PK, true>), dim3(grid), dim3(kTallBlock), 0, ctx->stream, view, st, p,
                                   V, X, S, Z, ctx->partials2));
  *count = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int tall_gram(mi_ctx *ctx, size_t n, int p, int variant, bool sym, const double *X, const double *Z, const double *dinv,
              double *out, int *count) {
  const int grid = row_grid_tall(ctx, n);
#define TG(VAR, SYM) \
  hipLaunchKernelGGL((k_tall_gram<VAR, SYM>), dim3(grid), dim3(kTallBlock), 0, ctx->stream, n, p, X, Z, dinv, out, ctx->partials2)
  if (variant == 0 && !sym) TG(0, false);
  else if (variant == 0) TG(0, true);
  else if (variant == 1) TG(1, true);
  else TG(2, true);
#undef TG
  *count = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int tall_reduce(mi_ctx *ctx, int count) {
  KScope ks(ctx, MI_K_STIEFEL_GRAM_REDUCE);
  // (p = 16: every entry of the tile is summed; entries outside a narrower Gram are zero in every row)
  hipLaunchKernelGGL(k_tall_reduce, dim3(1), dim3(kTallTile), 0, ctx->stream, (const double *)ctx->partials2, count,
                     kMaxPTall, ctx->partials2 + (size_t)kTallRows * kTallTile);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int tall_finish(mi_ctx *ctx, size_t n, int p, const CgState *st, const double *X, const double *Z, const double *Vin,
                int count, double *M_out, double *out, bool dots, int *nparts) {
  const double *rows = nullptr;
  int nrows = 0;
  MI_TRY(consumer_rows(ctx, count, &rows, &nrows));
  const int grid = row_grid_tall(ctx, n);
  KScope ks(ctx, MI_K_STIEFEL_FINISH_DOTS);
  DISPATCH_FLAG(dots, D,
                hipLaunchKernelGGL((k_tall_finish<D>), dim3(grid), dim3(kTallBlock), 0, ctx->stream, n, p, st, X, Z, Vin, rows,
                                   nrows, M_out, out, ctx->partials));
  if (nparts) *nparts = grid;
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int tall_polar(mi_ctx *ctx, size_t n, int p, double *Y, int count) {
  const double *rows = nullptr;
  int nrows = 0;
  MI_TRY(consumer_rows(ctx, count, &rows, &nrows));
  hipLaunchKernelGGL(k_tall_polar, dim3(row_grid_tall(ctx, n)), dim3(kTallBlock), 0, ctx->stream, n, p, Y, rows, nrows);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
