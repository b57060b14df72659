// stiefel_wide.h -- the one-pass Stiefel Hessian for rows wider than 4 doubles (p = 5 ... 8; the window form also serves
// p = 4), in three forms: k_st_hess_wide (one lane per row, sell_stream), k_st_hess_widewin (near rows from an LDS ring,
// sell_window) and k_st_hess_wideq (four lanes per row, sell_stream_quad).  Which one runs is decided by stiefel.hip's
// st_hess_plan from p, the matrix's window and MI355OPT_WIDE_WINDOW / MI355OPT_WIDE_QUAD.  A section of stiefel.hip's
// translation unit: included there once, inside its unnamed namespace, behind k_st_hess_fused.  It expects from what
// precedes it there: wide_sched and StChunk (stiefel.hip), SymIdx and DirComps (stiefel_core.h), sell_stream,
// sell_stream_quad, sell_window, QuadCols and pinned_load (spmm_core.h), HaloWaitArg / halo_wait (comm_ipc.h),
// block_partials_store_nw, wave_reduce_sum, xcd_remap, CgState and the SLOT_* indices (mi_internal.h).
#pragma once

// ---- rows wider than 4 doubles (p = 5 ... 8) ------------------------------------------------------------------------------
// The one-pass Hessian in its recurrence form for wide rows.  Same schedule and the same per-row arithmetic as
// k_st_hess_fused<P, ., ., RECUR = true, ...> -- Z = A V - V S, out = Z - X M with M = G(p) from STPCG's recurrence, the
// three curvature dots and the packed Gram sym(Y'out - (X'out) S) of the output in the epilogue of the only pass -- but
// laid out for what p = 8 costs: a row is 64 bytes, three P x P products per row, 3 + P (P + 1) / 2 <= 39 accumulators
// per lane.  So: 256-thread workgroups (one wave per SIMD, the whole vector register file to itself instead of the 128
// registers a 1024-thread workgroup leaves a wave), S and M in LDS (every lane reads the same address: broadcast reads,
// no bank conflicts) instead of 2 x 64 replicated registers, up to kMaxRows partial rows.
constexpr int kWideBlock = 256, kWideWaves = kWideBlock / 64;
// first slice of workgroup lb's range: the planned runs of whole 4-slice tiles (sparse.hip window_bounds: cut so that
// the far stride of the matrix -- the plane stride of a 3-D stencil -- is a whole number of runs, a far row then is
// some other workgroup's own row at the same moment of the kernel) or equal shares
__device__ __forceinline__ size_t wide_first_slice(size_t nslices, unsigned lb, unsigned nb, const int *bounds) {
  if (bounds) {
    const size_t s = (size_t)bounds[lb] * kWideWaves;
    return s < nslices ? s : nslices;
  }
  return (nslices * lb) / nb;
}
// waves per SIMD the wide kernels are held to (three would fit at p <= 7 and are slower: EXPERIMENTS.md "Decided knobs")
constexpr int kWideWavesPerSimd = 2;
template <int P, bool HALO, bool PK>
__global__ __launch_bounds__(kWideBlock) __attribute__((amdgpu_waves_per_eu(kWideWavesPerSimd, kWideWavesPerSimd))) void k_st_hess_wide(SellView A, const CgState *__restrict__ st,
                                                             const double *__restrict__ V, const double *__restrict__ X,
                                                             const double *__restrict__ Y, const double *__restrict__ S,
                                                             const double *__restrict__ gdir, double *__restrict__ out,
                                                             double *__restrict__ partials, HaloWaitArg<HALO> hwait,
                                                             const int *__restrict__ bounds) {
  constexpr int NS = SymIdx<P>::NS, KC = 3 + NS;
  __shared__ double lds[KC * kWideWaves];
  __shared__ double vt[PK ? 256 : 1];
  __shared__ double Sm[P * P], Mm[P * P];
  if (st && st->mode != CG_RUN) return;
  if constexpr (HALO) halo_wait(hwait.w);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (PK) vt[threadIdx.x] = A.vtab[threadIdx.x];
  if (threadIdx.x < P * P) {
    const int aa = threadIdx.x / P, b = threadIdx.x % P;
    Sm[threadIdx.x] = S[threadIdx.x];
    Mm[threadIdx.x] = gdir[SLOT_GDIR_P + (aa <= b ? SymIdx<P>::at(aa, b) : SymIdx<P>::at(b, aa))];
  }
  __syncthreads();
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t s0 = wide_first_slice(A.nslices, lb, nb, bounds), s1 = wide_first_slice(A.nslices, lb + 1, nb, bounds);
  double a[KC];
#pragma unroll
  for (int i = 0; i < KC; ++i) a[i] = 0;
  struct Epi {
    const SellView &A;
    const double *__restrict__ X, *__restrict__ Y, *__restrict__ V;
    double *__restrict__ out;
    const double *Sm, *Mm;
    double (&a)[KC];
    int lane;
    double x[P], y[P], v[P];
    __device__ __forceinline__ unsigned lane_off(size_t slice) const {
      return ((unsigned)slice * 64u + (unsigned)lane < (unsigned)A.n) ? (unsigned)lane * (unsigned)(P * 8) : 0u;
    }
    __device__ __forceinline__ const double *row_of(const double *F, size_t slice, unsigned off) const {
      return reinterpret_cast<const double *>(reinterpret_cast<const char *>(F) + (unsigned)slice * (unsigned)(64 * P * 8) + off);
    }
    __device__ __forceinline__ void begin(size_t slice) {
      const unsigned off = lane_off(slice);
      const double *xs = row_of(X, slice, off), *vs = row_of(V, slice, off), *ys = row_of(Y, slice, off);
#pragma unroll
      for (int c = 0; c < P; ++c) { x[c] = xs[c]; v[c] = vs[c]; y[c] = ys[c]; }
    }
    __device__ __forceinline__ void end(size_t slice, double (&acc)[P]) {
      if ((unsigned)slice * 64u + (unsigned)lane >= (unsigned)A.n) return;
      // (S and M are re-read from LDS for every row: loop-invariant code motion must not park 128 doubles in registers)
      asm volatile("" ::: "memory");
      double *os = reinterpret_cast<double *>(reinterpret_cast<char *>(out) + (unsigned)slice * (unsigned)(64 * P * 8) +
                                              lane_off(slice));
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += v[aa] * Sm[aa * P + b];
        acc[b] -= t;  // Z = A V - V S
        wide_sched();
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
        wide_sched();
      }
      double os_[P];  // packed sym(y o' - x (o S)'): the Gram of this output row
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += o[aa] * Sm[aa * P + b];
        os_[b] = t;
        wide_sched();
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
  } epi{A, X, Y, V, out, Sm, Mm, a, lane, {}, {}, {}};
  const int wu = __builtin_amdgcn_readfirstlane(w);
  sell_stream<P, HALO, PK, Epi, kWideWaves, StChunk<P>::value>(A, s0 + (size_t)wu, s1, lane, V, vt, epi);
  block_partials_store_nw<KC, kWideWaves>(a, lds, partials);
}

// The wide-row pass in WINDOW form (r06): the same epilogue as k_st_hess_wide (S and M in LDS, 3 + P (P +
// 1) / 2 partial components), but the product A V through spmm_core.h's sell_window instead of sell_stream -- the near
// rows of V come out of an LDS ring that is filled by coalesced 512-byte loads of whole 64-row chunks (a chunk of a
// row-major field is 64 P contiguous doubles), only the two far rows of a row are gathered lane by lane, and the far
// columns are computed (pure far structure).  What the lane-per-row form pays for -- seven neighbour gathers of P
// strided 8-byte loads each, every wave instruction touching 64 half-lines (profiles/r05_wide_ablation.txt) -- is gone;
// the own X and Y rows remain lane-per-row loads.  One context, packed matrix with a window (sparse.hip build_window),
// no halo.  The ring is dynamic LDS sized for the matrix's own window: (nc 64 + 1 + far slots) P doubles.

// workgroups per CU (= waves per SIMD) of the window form, p = 4 ... 8: two (256 VGPRs) up to p = 7, one at p = 8; three
// at p = 4 and one at p = 7 bought nothing (EXPERIMENTS.md "Decided knobs")
constexpr int wide_win_waves(int p) { return p <= 7 ? 2 : 1; }
// ring rows of the wide window form (spmm_core.h sell_window RS): at P = 8 rows 64 bytes apart put the row-by-row reads
// of a wave on a sixteenth of the LDS banks (218 us; 9 doubles apart: 102 us -- still behind the quad layout's 80, so
// p = 8 does not take this form by default); at P = 6 the padding changes nothing (57.7 us either way) and costs
// 11-14 registers: not applied
template <int P>
struct WideRing {
  static constexpr int stride = (P == 8) ? 9 : P;
};
template <int P, int HW, bool FARD>
__global__ __launch_bounds__(kWinBlock) __attribute__((amdgpu_waves_per_eu(wide_win_waves(P), wide_win_waves(P)))) void k_st_hess_widewin(
    SellView A, WinView Wv, const CgState *__restrict__ st, const double *__restrict__ V, const double *__restrict__ X,
    const double *__restrict__ Y, const double *__restrict__ S, const double *__restrict__ gdir, double *__restrict__ out,
    double *__restrict__ partials) {
  static_assert(kWideWaves == kWinWaves, "one workgroup shape");
  constexpr int KC = DirComps<P>::value;  // 3 + P (P + 1) / 2 (P = 4: padded to 16, the pads stay zero)
  __shared__ double lds[KC * kWideWaves];
  __shared__ double vt[256];
  __shared__ double Sm[P * P], Mm[P * P];
  extern __shared__ __attribute__((aligned(16))) double ring_dyn[];
  if (st && st->mode != CG_RUN) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  vt[threadIdx.x] = A.vtab[threadIdx.x];
  if (threadIdx.x < P * P) {
    const int aa = threadIdx.x / P, b = threadIdx.x % P;
    Sm[threadIdx.x] = S[threadIdx.x];
    Mm[threadIdx.x] = gdir[SLOT_GDIR_P + (aa <= b ? SymIdx<P>::at(aa, b) : SymIdx<P>::at(b, aa))];
  }
  // (sell_window's barrier behind the ring fill publishes vt, Sm and Mm too)
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  double a[KC];
#pragma unroll
  for (int i = 0; i < KC; ++i) a[i] = 0;
  struct Epi {
    const SellView &A;
    const double *__restrict__ X, *__restrict__ Y;
    double *__restrict__ out;
    const double *Sm, *Mm;
    double (&a)[KC];
    int lane;
    double xn[P], yn[P];
    __device__ __forceinline__ unsigned lane_off(size_t slice) const {
      return ((unsigned)slice * 64u + (unsigned)lane < (unsigned)A.n) ? (unsigned)lane * (unsigned)(P * 8) : 0u;
    }
    __device__ __forceinline__ const double *row_of(const double *F, size_t slice, unsigned off) const {
      return reinterpret_cast<const double *>(reinterpret_cast<const char *>(F) + (unsigned)slice * (unsigned)(64 * P * 8) + off);
    }
    // P = 4, 6: a row is two / three 16-byte pieces -- P / 2 global_load_dwordx4 per field instead of P 8-byte loads (half
    // the texture-path instructions, half the hits on lines still pending; slower at P = 8: EXPERIMENTS.md "Decided
    // knobs").  There is no ordered (pinned) 16-byte load to be had from the compiler, so these are asm statements:
    // absent from hipcc's s_waitcnt bookkeeping, waited for by the explicit vmcnt(0) in arrive() (they are the newest
    // loads of the tile: a wait hipcc computes for an older load only gets longer).
    typedef double v2d __attribute__((ext_vector_type(2)));
    v2d xq[3], yq[3];
    __device__ __forceinline__ void request(size_t slice) {
      if constexpr (P == 4 || P == 6) {
        const unsigned off = (unsigned)slice * (unsigned)(64 * P * 8) + lane_off(slice);
#pragma unroll
        for (int c = 0; c < P / 2; ++c)
          asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(xq[c]) : "v"(off), "s"(X), "n"(16 * c) : "memory");
#pragma unroll
        for (int c = 0; c < P / 2; ++c)
          asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(yq[c]) : "v"(off), "s"(Y), "n"(16 * c) : "memory");
      } else {
        const unsigned off = lane_off(slice);
        const double *xs = row_of(X, slice, off), *ys = row_of(Y, slice, off);
#pragma unroll
        for (int c = 0; c < P; ++c) xn[c] = pinned_load(xs + c);
#pragma unroll
        for (int c = 0; c < P; ++c) yn[c] = pinned_load(ys + c);
      }
    }
    __device__ __forceinline__ void arrive() {
      if constexpr (P == 6)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xq[0]), "+v"(xq[1]), "+v"(xq[2]), "+v"(yq[0]), "+v"(yq[1]), "+v"(yq[2])::"memory");
      else if constexpr (P == 4)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xq[0]), "+v"(xq[1]), "+v"(yq[0]), "+v"(yq[1])::"memory");
      if constexpr (P == 4 || P == 6) {
#pragma unroll
        for (int c = 0; c < P / 2; ++c) { xn[2 * c] = xq[c].x; xn[2 * c + 1] = xq[c].y; yn[2 * c] = yq[c].x; yn[2 * c + 1] = yq[c].y; }
      }
    }
    __device__ __forceinline__ void end(size_t slice, double (&acc)[P], const double (&v)[P]) {
      arrive();  // (every lane: the wait is not a matter of the lane's row)
      if ((unsigned)slice * 64u + (unsigned)lane >= (unsigned)A.n) return;
      // (S and M are re-read from LDS for every row: loop-invariant code motion must not park 128 doubles in registers)
      asm volatile("" ::: "memory");
      double *os = reinterpret_cast<double *>(reinterpret_cast<char *>(out) + (unsigned)slice * (unsigned)(64 * P * 8) +
                                              lane_off(slice));
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += v[aa] * Sm[aa * P + b];
        acc[b] -= t;  // Z = A V - V S
        wide_sched();
      }
      double o[P];
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += xn[aa] * Mm[aa * P + b];
        o[b] = acc[b] - t;  // Z - X M
        os[b] = o[b];  // (non-temporal stores / loads of the own rows: 58 -> 63-74 us at p = 6, EXPERIMENTS.md r06)
        a[0] += v[b] * o[b]; a[1] += o[b] * o[b]; a[2] += v[b] * v[b];
        wide_sched();
      }
      double os_[P];  // packed sym(y o' - x (o S)'): the Gram of this output row
#pragma unroll
      for (int b = 0; b < P; ++b) {
        double t = 0;
#pragma unroll
        for (int aa = 0; aa < P; ++aa) t += o[aa] * Sm[aa * P + b];
        os_[b] = t;
        wide_sched();
      }
#pragma unroll
      for (int aa = 0; aa < P; ++aa)
#pragma unroll
        for (int b = aa; b < P; ++b) {
          const double gab = yn[aa] * o[b] - xn[aa] * os_[b];
          const double gba = yn[b] * o[aa] - xn[b] * os_[aa];
          a[3 + SymIdx<P>::at(aa, b)] += (aa == b) ? gab : .5 * (gab + gba);
        }
    }
  } epi{A, X, Y, out, Sm, Mm, a, lane, {}, {}};
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const int ntiles = (int)((A.nslices + kWinWaves - 1) / kWinWaves), per = (ntiles + (int)nb - 1) / (int)nb;
  int t0 = (int)lb * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  if (Wv.bounds) {
    t0 = scalar_int(Wv.bounds, lb);
    t1 = scalar_int(Wv.bounds, lb + 1);
  }
  if (t0 >= t1) __syncthreads();  // (sell_window returns at once: the tables above still need their barrier)
  sell_window<P, HW, false, FARD, false, Epi, WideRing<P>::stride, FARD>(A, Wv, t0, t1, wu, lane, V, vt, ring_dyn, epi);
  __syncthreads();
  block_partials_store_nw<KC, kWideWaves>(a, lds, partials);
}

// The same pass in the QUAD layout of spmm_core.h (sell_stream_quad): lane (g, q) holds columns 2q, 2q + 1 of the rows
// 16 t + g of its wave's slice, every load and store of a row is 64 contiguous bytes per quad.  A row's full width --
// the left operands of the three products and of the Gram -- comes from the quad's four lanes by DPP broadcasts; S and M
// sit in LDS padded to 8 x 8 with zero columns (a lane reads its two columns of a row of the matrix as one 16-byte
// read); the Gram of the output is accumulated RAW (y_a o_b - x_a (o S)_b for the lane's two b: 2 P accumulators instead
// of P (P + 1) / 2) and symmetrised once, at the end, through LDS.
template <int CTRL>
__device__ __forceinline__ double dpp_quad_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
// full[2 i + c] = the value of column 2 i + c held by lane i of the quad
template <int P>
__device__ __forceinline__ void quad_row(const double (&own)[2], double (&full)[8]) {
  full[0] = dpp_quad_f64<0x00>(own[0]); full[1] = dpp_quad_f64<0x00>(own[1]);
  full[2] = dpp_quad_f64<0x55>(own[0]); full[3] = dpp_quad_f64<0x55>(own[1]);
  full[4] = dpp_quad_f64<0xAA>(own[0]);
  if constexpr (P > 5) full[5] = dpp_quad_f64<0xAA>(own[1]);
  if constexpr (P > 6) full[6] = dpp_quad_f64<0xFF>(own[0]);
  if constexpr (P > 7) full[7] = dpp_quad_f64<0xFF>(own[1]);
}
constexpr int kWideQuadChunk = 8;  // entries per chunk step of the quad-layout pass (16 bytes per entry and lane)
template <int P, bool HALO, bool PK>
__global__ __launch_bounds__(kWideBlock) __attribute__((amdgpu_waves_per_eu(kWideWavesPerSimd, kWideWavesPerSimd))) void k_st_hess_wideq(SellView A, const CgState *__restrict__ st,
                                                             const double *__restrict__ V, const double *__restrict__ X,
                                                             const double *__restrict__ Y, const double *__restrict__ S,
                                                             const double *__restrict__ gdir, double *__restrict__ out,
                                                             double *__restrict__ partials, HaloWaitArg<HALO> hwait,
                                                             const int *__restrict__ bounds) {
  constexpr int NS = SymIdx<P>::NS, KC = 3 + NS;
  __shared__ double lds[3 * kWideWaves];
  __shared__ double graw[kWideWaves][P][8];
  __shared__ double vt[PK ? 256 : 1];
  __shared__ __attribute__((aligned(16))) double Sm[P * 8], Mm[P * 8];
  if (st && st->mode != CG_RUN) return;
  if constexpr (HALO) halo_wait(hwait.w);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (PK) vt[threadIdx.x] = A.vtab[threadIdx.x];
  if (threadIdx.x < P * 8) {
    const int aa = threadIdx.x >> 3, b = threadIdx.x & 7;
    Sm[threadIdx.x] = b < P ? S[aa * P + b] : 0.0;
    Mm[threadIdx.x] = b < P ? gdir[SLOT_GDIR_P + (aa <= b ? SymIdx<P>::at(aa, b) : SymIdx<P>::at(b, aa))] : 0.0;
  }
  __syncthreads();
  const unsigned nb = gridDim.x, lb = xcd_remap(blockIdx.x, nb);
  const size_t s0 = wide_first_slice(A.nslices, lb, nb, bounds), s1 = wide_first_slice(A.nslices, lb + 1, nb, bounds);
  double a[3] = {0, 0, 0};
  double G[P][2];
#pragma unroll
  for (int i = 0; i < P; ++i) G[i][0] = G[i][1] = 0;
  struct Epi {
    const SellView &A;
    const double *__restrict__ X, *__restrict__ Y, *__restrict__ V;
    double *__restrict__ out;
    const double *Sm, *Mm;
    double (&a)[3];
    double (&G)[P][2];
    int q, g;
    unsigned o0, o1;
    __device__ __forceinline__ unsigned row_off(size_t slice, int t) const {  // (rows past the end re-read the slice's first)
      const unsigned r = (unsigned)slice * 64u + (unsigned)(16 * t + g);
      return (r < (unsigned)A.n ? r : (unsigned)slice * 64u) * (unsigned)(P * 8);
    }
    __device__ __forceinline__ void begin(size_t slice, int t, double (&x)[2], double (&v)[2], double (&y)[2]) const {
      const unsigned off = row_off(slice, t);
      QuadCols<P>::load(reinterpret_cast<const char *>(X), off, o0, o1, x[0], x[1]);
      QuadCols<P>::load(reinterpret_cast<const char *>(V), off, o0, o1, v[0], v[1]);
      QuadCols<P>::load(reinterpret_cast<const char *>(Y), off, o0, o1, y[0], y[1]);
    }
    __device__ __forceinline__ void end(size_t slice, int t, double (&acc)[2], const double (&x)[2], const double (&v)[2],
                                        const double (&y)[2]) {
      const bool c0 = 2 * q < P, c1 = 2 * q + 1 < P;
      const double2 *S2 = reinterpret_cast<const double2 *>(Sm) + q, *M2 = reinterpret_cast<const double2 *>(Mm) + q;
      // (S and M are re-read from LDS for every row: loop-invariant code motion must not park them in registers)
      asm volatile("" ::: "memory");
      const bool live = (unsigned)slice * 64u + (unsigned)(16 * t + g) < (unsigned)A.n;
      const bool u0 = live && c0, u1 = live && c1;
      const double vv[2] = {u0 ? v[0] : 0.0, u1 ? v[1] : 0.0};
      const double xx[2] = {u0 ? x[0] : 0.0, u1 ? x[1] : 0.0};
      const double yy[2] = {u0 ? y[0] : 0.0, u1 ? y[1] : 0.0};
      double z[2] = {u0 ? acc[0] : 0.0, u1 ? acc[1] : 0.0};
      double vf[8], xf[8], yf[8], of[8];
      quad_row<P>(vv, vf);
      quad_row<P>(xx, xf);
#pragma unroll
      for (int aa = 0; aa < P; ++aa) {  // Z = A V - V S, then out = Z - X M (the lane's two columns)
        const double2 sc = S2[aa * 4];
        z[0] -= vf[aa] * sc.x; z[1] -= vf[aa] * sc.y;
      }
      wide_sched();
#pragma unroll
      for (int aa = 0; aa < P; ++aa) {
        const double2 mc = M2[aa * 4];
        z[0] -= xf[aa] * mc.x; z[1] -= xf[aa] * mc.y;
      }
      wide_sched();
      {
        char *ob = reinterpret_cast<char *>(out);
        const unsigned ro = row_off(slice, t);
        if constexpr (P % 2 == 0) {
          if (u0) *reinterpret_cast<double2 *>(ob + (ro + o0)) = make_double2(z[0], z[1]);
        } else {
          if (u0) *reinterpret_cast<double *>(ob + (ro + o0)) = z[0];
          if (u1) *reinterpret_cast<double *>(ob + (ro + o1)) = z[1];
        }
      }
      a[0] += vv[0] * z[0]; a[0] += vv[1] * z[1];
      a[1] += z[0] * z[0]; a[1] += z[1] * z[1];
      a[2] += vv[0] * vv[0]; a[2] += vv[1] * vv[1];
      quad_row<P>(z, of);
      double os_[2] = {0, 0};  // (o S), the lane's two columns
#pragma unroll
      for (int aa = 0; aa < P; ++aa) {
        const double2 sc = S2[aa * 4];
        os_[0] += of[aa] * sc.x; os_[1] += of[aa] * sc.y;
      }
      wide_sched();
      quad_row<P>(yy, yf);
#pragma unroll
      for (int aa = 0; aa < P; ++aa) {  // raw Gram of this output row: y_a o_b - x_a (o S)_b
        G[aa][0] += yf[aa] * z[0] - xf[aa] * os_[0];
        G[aa][1] += yf[aa] * z[1] - xf[aa] * os_[1];
      }
    }
  } epi{A, X, Y, V, out, Sm, Mm, a, G, lane & 3, lane >> 2, QuadCols<P>::off0(lane & 3), QuadCols<P>::off1(lane & 3)};
  const int wu = __builtin_amdgcn_readfirstlane(w);
  sell_stream_quad<P, HALO, PK, Epi, kWideWaves, kWideQuadChunk>(A, s0 + (size_t)wu, s1, lane, V, vt, epi);
  // the wave's raw Gram: sum over the 16 quads (lane bits 2..5), lanes 0..3 hold columns 2q, 2q + 1
#pragma unroll
  for (int aa = 0; aa < P; ++aa)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      double t = G[aa][c];
#pragma unroll
      for (int m = 4; m < 64; m <<= 1) t += __shfl_xor(t, m, 64);
      if (lane < 4) graw[w][aa][2 * lane + c] = t;
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t = wave_reduce_sum(a[k]);
    if (lane == 0) lds[k * kWideWaves + w] = t;
  }
  __syncthreads();
  if (threadIdx.x < KC) {
    double t[kWideWaves];
    if (threadIdx.x < 3) {
#pragma unroll
      for (int i = 0; i < kWideWaves; ++i) t[i] = lds[threadIdx.x * kWideWaves + i];
    } else {
      int aa = 0, idx = (int)threadIdx.x - 3;  // packed index -> (aa, b), aa <= b
      while (idx >= P - aa) { idx -= P - aa; ++aa; }
      const int b = aa + idx;
#pragma unroll
      for (int i = 0; i < kWideWaves; ++i) t[i] = aa == b ? graw[i][aa][aa] : .5 * (graw[i][aa][b] + graw[i][b][aa]);
    }
#pragma unroll
    for (int span = 1; span < kWideWaves; span *= 2)
#pragma unroll
      for (int i = 0; i + span < kWideWaves; i += 2 * span) t[i] = t[i] + t[i + span];
    partials[(size_t)threadIdx.x * kMaxRows + blockIdx.x] = t[0];
  }
}
