// stpcg.hip -- fused device realisation of Optimization::LinearAlgebra::STPCG
// (reference: LinearAlgebra/IterativeSolvers.h:166-426, unconstrained form).
//
// Design (MI355X-first):
//   * every vector phase between two global reductions is ONE streaming kernel (16 B/lane loads,
//     <= 512 fat workgroups, grid-stride) that ends by writing one partial-sum row per workgroup;
//   * there are NO scalar kernels in the loop: the next streaming kernel's workgroups each re-reduce
//     those <= 512 rows in their prologue (identical code on identical data => bit-identical totals
//     in every workgroup, deterministic, no fp64 atomics) and each advance the reference's scalar
//     recurrences (:259-283,330-345,412-417) and take its branch decisions themselves; workgroup 0
//     persists the new state.  The state is double-buffered (read st_in, write st_out) so no
//     workgroup can observe a half-updated state;
//   * the host never reads a scalar back inside the loop: it enqueues iterations speculatively,
//     bounded by `run_ahead`, and watches a pinned progress word; kernels enqueued past the exit see
//     mode == CG_DONE and return immediately;
//   * row-sharded multi-GPU: partial rows -> one-workgroup reduce -> in-stream RCCL all-reduce ->
//     the consumers read the all-reduced slots instead (the recurrences are replicated; every rank
//     takes identical decisions because ncclAllReduce returns identical bits everywhere).
//
// Per completed iteration the CG part launches 2 kernels:
//   k_cg_update   A-step prologue (kappa, kernel test, alpha, boundary test :300-362) +
//                 s += alpha p, r += alpha Hp, v = M^-1 r, partial <r,v> (:374-408)      [6N (+2N/+4N)]
//   k_cg_pupdate  B-step prologue (beta, M-norm recurrences, loop control :408-417,285,290) +
//                 p = -v + beta p (:420)                                                [3N]
// and the operator supplies <p,Hp>, <Hp,Hp>, <p,p> partials from its last pass (else k_cg_dot3, 2N).
#include "comm_ipc.h"
#include "mi_internal.h"
#include "stiefel_core.h"

#include <cmath>
#include <type_traits>

using namespace mi;

namespace {

enum { PRE_NONE = 0, PRE_DIAG = 1, PRE_BLOCK3 = 2, PRE_EXTERNAL = 3 };

__device__ __forceinline__ void publish(HostStatus *hs, unsigned long long launches, int done) {
  // one relaxed system-scope store: the host only looks at this word (results are read after a stream
  // synchronisation), so no release/write-back of the L2 is needed here
  __hip_atomic_store(&hs->word, (uint64_t)(launches << 1) | (uint64_t)(done ? 1 : 0), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

// Field-by-field state copies.  An aggregate copy (`*dst = cs`) makes the compiler keep the
// per-thread struct in memory (promoted to 56 B/thread of LDS + scratch: +7-10 us per kernel,
// tools/microbench/prologue.hip); explicit fields let SROA keep everything in registers.
#define CG_FIELDS(X)                                                                               \
  X(sk_M_pk) X(sk_M_2) X(pk_M_2) X(target_rk_norm) X(rv) X(alpha) X(beta)                          \
  X(kappa) X(sigma) X(skplus1_M_2) X(M_norm) X(k) X(launches) X(mode) X(exit_reason)
__device__ __forceinline__ CgState load_state(const CgState *__restrict__ src) {
  CgState s;
#define X(f) s.f = src->f;
  CG_FIELDS(X)
#undef X
  return s;
}
__device__ __forceinline__ void store_state(CgState *__restrict__ dst, const CgState &s) {
#define X(f) dst->f = s.f;
  CG_FIELDS(X)
#undef X
}

// ---------------------------------------------------------------------------------------------
// scalar steps.  fp contraction is off so the recurrences round exactly like the reference's
// scalar C++ on the host.
// ---------------------------------------------------------------------------------------------

// after the operator: kappa, kernel test, alpha, boundary test (:300-362)
__device__ __forceinline__ void step_a(CgState &s, const CgConst &c, double pHp, double HpHp, double pp) {
#pragma clang fp contract(off)
  const double kappa = pHp;  // :300
  s.kappa = kappa;
  if (sqrt(HpHp) / sqrt(pp) < c.epsilon) {  // :305-307
    s.mode = CG_KERNEL_PENDING;              // needs <p,r> (:320): supplied by k_cg_update's body
    return;
  }
  const double alpha = s.rv / kappa;                                               // :341
  const double skplus1 = s.sk_M_2 + 2 * alpha * s.sk_M_pk + alpha * alpha * s.pk_M_2;  // :344-345
  if ((kappa <= 0) || (skplus1 > c.Delta_2)) {                                     // :347
    s.sigma = (-s.sk_M_pk + sqrt(s.sk_M_pk * s.sk_M_pk + s.pk_M_2 * (c.Delta_2 - s.sk_M_2))) /
              s.pk_M_2;  // :355-357
    s.mode = CG_APPLY_SIGMA;
    s.exit_reason = MI_STPCG_EXIT_BOUNDARY;
    return;
  }
  s.alpha = alpha;
  s.skplus1_M_2 = skplus1;
}

// after the update: resolves every mode; returns true if a direction update p = -v + beta p follows
__device__ __forceinline__ void step_b(CgState &s, const CgConst &c, double red) {
#pragma clang fp contract(off)
  if (s.mode == CG_APPLY_SIGMA) {  // boundary step applied by k_cg_update (:359-361)
    s.M_norm = c.Delta;
    s.mode = CG_DONE;
    return;
  }
  if (s.mode == CG_KERNEL_PENDING) {  // :320-337, red = <p,r>
    double sk_M_pk = s.sk_M_pk;
    const bool flip = red < 0;
    if (flip) sk_M_pk *= -1;  // :325
    const double sigma =
        (-sk_M_pk + sqrt(sk_M_pk * sk_M_pk + s.pk_M_2 * (c.Delta_2 - s.sk_M_2))) / s.pk_M_2;  // :330
    s.sk_M_pk = sk_M_pk;
    s.sigma = flip ? -sigma : sigma;  // s += sigma * (-p)  ==  s += (-sigma) * p   (:324,336)
    s.M_norm = c.Delta;               // :334
    s.exit_reason = MI_STPCG_EXIT_KERNEL;
    s.mode = CG_DONE;                 // k_cg_pupdate's body applies the step
    return;
  }
  // CG_RUN, red = <r,v> after the update
  const double rk_vk = red;                                  // :408
  const double beta = rk_vk / (s.alpha * s.kappa);           // :412
  s.sk_M_2 = s.skplus1_M_2;                                  // :415
  s.sk_M_pk = beta * (s.sk_M_pk + s.alpha * s.pk_M_2);       // :416
  s.pk_M_2 = rk_vk + beta * beta * s.pk_M_2;                 // :417
  s.rv = rk_vk;
  s.beta = beta;
  s.k = s.k + 1;
  if (s.k >= c.max_iterations) {  // :285
    s.exit_reason = MI_STPCG_EXIT_MAXIT;
    s.M_norm = sqrt(s.sk_M_2);  // :424
    s.mode = CG_DONE;
  } else if (sqrt(rk_vk) <= s.target_rk_norm) {  // :290 (top of the next pass)
    s.exit_reason = MI_STPCG_EXIT_RESIDUAL;
    s.M_norm = sqrt(s.sk_M_2);
    s.mode = CG_DONE;
  }
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// r'-halo form of the sharded solve (comm_ipc.h comm_rprime_*): halo(p') = -halo(r') + beta halo(p), the expression
// k_cg_pupdate evaluates for the rows it owns (:420) -- same TU, same contraction, same bits -- applied by every rank to
// the halo rows it holds.  `st` is the state k_cg_pupdate left: a direction update happened iff it still says CG_RUN.
__global__ __launch_bounds__(256) void k_halo_dir(const CgState *__restrict__ st, const double *__restrict__ hr,
                                                  double *__restrict__ hp, size_t count) {
  if (st->mode != CG_RUN) return;
  const double beta = st->beta;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256)
    hp[i] = -hr[i] + beta * hp[i];
}


// r = g; s = 0*g (:211,214); v = P r (:231/234); p = -v (:256); partial <r,v> (:266)
template <int PRE>
__global__ __launch_bounds__(kBlock) void k_cg_init(size_t n, const double *__restrict__ g,
                                                    const double *__restrict__ pre,
                                                    double *__restrict__ r, double *__restrict__ v,
                                                    double *__restrict__ p, double *__restrict__ s,
                                                    double *__restrict__ partials) {
  __shared__ double lds[kWaves];
  double acc[1] = {0};
  const size_t stride = (size_t)gridDim.x * kBlock;
  if (PRE == PRE_BLOCK3) {
    const size_t nb = n / 3;
    for (size_t b = (size_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += stride) {
      const double g0 = g[3 * b], g1 = g[3 * b + 1], g2 = g[3 * b + 2];
      const double *M = pre + 9 * b;
      const double v0 = M[0] * g0 + M[1] * g1 + M[2] * g2;
      const double v1 = M[3] * g0 + M[4] * g1 + M[5] * g2;
      const double v2 = M[6] * g0 + M[7] * g1 + M[8] * g2;
      r[3 * b] = g0; r[3 * b + 1] = g1; r[3 * b + 2] = g2;
      s[3 * b] = 0 * g0; s[3 * b + 1] = 0 * g1; s[3 * b + 2] = 0 * g2;
      v[3 * b] = v0; v[3 * b + 1] = v1; v[3 * b + 2] = v2;
      p[3 * b] = -v0; p[3 * b + 1] = -v1; p[3 * b + 2] = -v2;
      acc[0] += g0 * v0; acc[0] += g1 * v1; acc[0] += g2 * v2;
    }
  } else {
    const size_t n2 = n >> 1;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) {
      const double2 gv = reinterpret_cast<const double2 *>(g)[i];
      reinterpret_cast<double2 *>(r)[i] = gv;
      reinterpret_cast<double2 *>(s)[i] = make_double2(0 * gv.x, 0 * gv.y);
      if (PRE == PRE_EXTERNAL) continue;
      double2 vv = gv;
      if (PRE == PRE_DIAG) {
        const double2 d = reinterpret_cast<const double2 *>(pre)[i];
        vv.x = d.x * gv.x; vv.y = d.y * gv.y;
        reinterpret_cast<double2 *>(v)[i] = vv;
      }
      reinterpret_cast<double2 *>(p)[i] = make_double2(-vv.x, -vv.y);
      acc[0] += gv.x * vv.x; acc[0] += gv.y * vv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      const size_t i = n - 1;
      const double gv = g[i];
      r[i] = gv; s[i] = 0 * gv;
      if (PRE != PRE_EXTERNAL) {
        double vv = gv;
        if (PRE == PRE_DIAG) { vv = pre[i] * gv; v[i] = vv; }
        p[i] = -vv;
        acc[0] += gv * vv;
      }
    }
  }
  if (PRE == PRE_EXTERNAL) return;
  block_partials_store<1>(acc, lds, partials);
}

// external preconditioner path: partial <r,v>; NEG_P: also p = -v (initialisation, :256)
template <bool NEG_P>
__global__ __launch_bounds__(kBlock) void k_cg_dot_rv(size_t n, const CgState *__restrict__ st,
                                                      const double *__restrict__ r,
                                                      const double *__restrict__ v,
                                                      double *__restrict__ p,
                                                      double *__restrict__ partials) {
  __shared__ double lds[kWaves];
  if (!NEG_P && st->mode != CG_RUN) return;  // the update kernel already left the partial it needs
  double acc[1] = {0};
  const size_t n2 = n >> 1, stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) {
    const double2 rv = reinterpret_cast<const double2 *>(r)[i];
    const double2 vv = reinterpret_cast<const double2 *>(v)[i];
    if (NEG_P) reinterpret_cast<double2 *>(p)[i] = make_double2(-vv.x, -vv.y);
    acc[0] += rv.x * vv.x; acc[0] += rv.y * vv.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    if (NEG_P) p[n - 1] = -v[n - 1];
    acc[0] += r[n - 1] * v[n - 1];
  }
  block_partials_store<1>(acc, lds, partials);
}

// partials of <x,y>, <y,y>, <x,x>  (kappa :300, kernel test :305-306) for operators without fused dots
__global__ __launch_bounds__(kBlock) void k_cg_dot3(size_t n, const CgState *__restrict__ st,
                                                    const double *__restrict__ x,
                                                    const double *__restrict__ y,
                                                    double *__restrict__ partials) {
  __shared__ double lds[3 * kWaves];
  if (st && st->mode != CG_RUN) return;
  double a[3] = {0, 0, 0};
  const size_t n2 = n >> 1, stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) {
    const double2 xv = reinterpret_cast<const double2 *>(x)[i];
    const double2 yv = reinterpret_cast<const double2 *>(y)[i];
    a[0] += xv.x * yv.x; a[0] += xv.y * yv.y;
    a[1] += yv.x * yv.x; a[1] += yv.y * yv.y;
    a[2] += xv.x * xv.x; a[2] += xv.y * xv.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double xv = x[n - 1], yv = y[n - 1];
    a[0] += xv * yv; a[1] += yv * yv; a[2] += xv * xv;
  }
  block_partials_store<3>(a, lds, partials);
}

// G(p0) (packed symmetric, gns components, wave w sums the `count` partial rows of components w, w + 16, ... in fixed order)
// into gdir[SLOT_GDIR_P..), and G(r0) = -G(p0) (p0 = -r0) into gdir[0..)
__device__ __forceinline__ void gdir_from_rows(const double *__restrict__ partials, int count, int gns,
                                               double *__restrict__ gdir) {
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x >> 6; w < gns; w += kWaves) {  // (gns > kWaves: p >= 6, in rounds)
    const double *src = partials + (size_t)w * kMaxRows;
    double t[kMaxRows / 64];
#pragma unroll
    for (int j = 0; j < kMaxRows / 64; ++j) {
      const int r = lane + 64 * j;
      t[j] = (r < count) ? src[r] : 0.0;
    }
    double v = 0;
#pragma unroll
    for (int j = 0; j < kMaxRows / 64; ++j) v += t[j];
    v = wave_reduce_sum(v);
    if (lane == 0) {
      gdir[SLOT_GDIR_P + w] = v;
      gdir[w] = -v;
    }
  }
}

// the same fixed-order reduction into ONE destination (re-anchoring, r06)
__device__ __forceinline__ void gdir_rows_to(const double *__restrict__ partials, int count, int gns,
                                             double *__restrict__ dst) {
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x >> 6; w < gns; w += kWaves) {
    const double *src = partials + (size_t)w * kMaxRows;
    double t[kMaxRows / 64];
#pragma unroll
    for (int j = 0; j < kMaxRows / 64; ++j) {
      const int r = lane + 64 * j;
      t[j] = (r < count) ? src[r] : 0.0;
    }
    double v = 0;
#pragma unroll
    for (int j = 0; j < kMaxRows / 64; ++j) v += t[j];
    v = wave_reduce_sum(v);
    if (lane == 0) dst[w] = v;
  }
}

struct CgSetup {
  double Delta, kappa_fgr, theta, epsilon;
  unsigned long long max_iterations;
};

// one workgroup, once per solve: :259-279 and the first pass of :285-290
// gdir != nullptr: k_cg_gdir_init's work rides along (one rank, recurrence form: its kernel has nothing to wait for):
// G(p0) from the `gcount` Gram rows k_cg_init_dirgram left, G(r0) = -G(p0)
template <bool FROM_SLOTS>
__global__ __launch_bounds__(kBlock) void k_cg_scalar_init(CgState *st, CgSetup cfg,
                                                           const double *partials, int nparts,
                                                           const double *slots, HostStatus *hs,
                                                           const double *__restrict__ gpartials, int gcount, int gns,
                                                           double *__restrict__ gdir) {
#pragma clang fp contract(off)
  __shared__ double lds[kWaves + 1];
  if (gdir) gdir_from_rows(gpartials, gcount, gns, gdir);
  double red[1];
  if (FROM_SLOTS) red[0] = slots[0];
  else reduce_rows<1>(partials, nparts, red, lds);
  if (threadIdx.x != 0) return;
  CgState s;
  const double rv0 = red[0];
  s.sk_M_pk = 0;                        // :259
  s.sk_M_2 = 0;                         // :263
  s.pk_M_2 = rv0;                       // :266
  const double r0_norm = sqrt(rv0);     // :275
  const double pw = pow(r0_norm, cfg.theta);
  s.target_rk_norm = r0_norm * ((pw < cfg.kappa_fgr) ? pw : cfg.kappa_fgr);  // :278-279 (std::min)
  s.rv = rv0;
  s.alpha = s.beta = s.kappa = s.sigma = s.skplus1_M_2 = 0;
  s.M_norm = 0;
  s.k = 0;
  s.launches = 0;
  s.exit_reason = MI_STPCG_EXIT_MAXIT;
  s.mode = CG_RUN;
  if (cfg.max_iterations == 0) {  // :285 body never runs
    s.mode = CG_DONE;
    s.M_norm = sqrt(0.0);  // :424
  } else if (sqrt(rv0) <= s.target_rk_norm) {  // :290
    s.mode = CG_DONE;
    s.exit_reason = MI_STPCG_EXIT_RESIDUAL;
    s.M_norm = sqrt(0.0);
  }
  store_state(st, s);
  publish(hs, 0, s.mode == CG_DONE);
}

// mi_op::dirgram plumbing.  Direct form: k_cg_pupdate<.,SP> forms the Gram rows of the new direction from X, Y.
// Recurrence form (gdir != null, no preconditioner): the operator pass leaves the rows of G(Hp) as components
// 3.. of its partial row; workgroup 0 of k_cg_update advances G(r) += alpha G(Hp) and workgroup 0 of
// k_cg_pupdate G(p) = -G(r) + beta G(p) -- packed symmetric, ns = P(P+1)/2 doubles each at gdir[0..) / gdir[SLOT_GDIR_P..).
struct DirGramArgs {
  const double *X, *Y, *S;
  double *gpartials;
  double *gdir;
  int ns;
};

// A-step prologue + body:
//   CG_RUN:            r += alpha Hp (:377); v = P r (:383/386); partial <r,v> (:408)   [s += alpha p: see k_cg_pupdate]
//   CG_APPLY_SIGMA:    s += sigma p (:360)
//   CG_KERNEL_PENDING: partial <p,r> (:320)
// (the kernels follow the DirGramLds helper below: stpcg_kernels.inc)
#ifdef MI_FOLD_STAMPS
}  // namespace
extern "C" __attribute__((visibility("default"))) int mi_debug_fold_stamp_buffer(void *dev_ptr) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(mi::g_fold_stamps), &dev_ptr, sizeof(dev_ptr));
}
namespace {
#endif

// B-step prologue + body:  CG_RUN: s = s + alpha p (:374), p = -v + beta p (:420);  kernel exit: s += sigma p (:336)
//   SP > 0 (mi_op::dirgram): the fields are rows of SP doubles and the kernel also leaves the partial rows of
//   sym(Y'p - (X'p) S) of the NEW direction in dg.gpartials -- the projection matrix of the next Hessian pass.
template <int SP>
struct DirGramLds {
  static constexpr int value = (SymIdx<SP>::NS * kWaves > kWaves + 1) ? SymIdx<SP>::NS * kWaves : kWaves + 1;
};
template <>
struct DirGramLds<0> {
  static constexpr int value = kWaves + 1;  // (>= kIpcVals: the folded exchange's staging)
};
static_assert(kWaves + 1 >= kIpcVals, "LDS of the folded exchange");

#define CG_KERNEL_ATTR
#define CG_UPDATE_SIGMA 1
#define CG_UPDATE_NAME k_cg_update
#define CG_PUPDATE_NAME k_cg_pupdate
#include "stpcg_kernels.inc"
#undef CG_KERNEL_ATTR
#undef CG_UPDATE_NAME
#undef CG_PUPDATE_NAME
// The same two kernels with at most 80 scalar registers.  Measured on gfx950 (tools/fold_stamps.py, in-kernel clock
// stamps): a kernel that is allocated 96 SGPRs gets 7 waves per SIMD, not the 8 the compiler reports -- and these
// kernels run 1024-thread workgroups, two per CU, which needs all 8: with 81..96 SGPRs the second half of the grid only
// starts when the first half has finished (k_cg_update: +3.7 us of 15).  The single-GPU instantiations of the hot loop
// sit at exactly 80; the ones that carry the exchange arguments (FoldArgs, FoldPush), read reduced slots, or keep 16
// components need 82..100 and are launched from this pair instead: a few scalar spills to vector lanes.
#define CG_KERNEL_ATTR __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8)))
#define CG_UPDATE_NAME k_cg_update_s80
#define CG_PUPDATE_NAME k_cg_pupdate_s80
#include "stpcg_kernels.inc"
#undef CG_KERNEL_ATTR
#undef CG_UPDATE_NAME
#undef CG_PUPDATE_NAME
#undef CG_UPDATE_SIGMA
// k_cg_update WITHOUT the boundary step's s += sigma p: the A-step of an odd iteration of the deferred-s form (below,
// k_cg_pupdate_ds), where the direction kernel behind it applies that step after the pending term.  A third and fourth
// inclusion, not a template parameter or a flag: the kernels above keep their code, their registers and their names.
// (the direction kernel of these inclusions is never instantiated)
#define CG_UPDATE_SIGMA 0
#define CG_KERNEL_ATTR
#define CG_UPDATE_NAME k_cg_update_ns
#define CG_PUPDATE_NAME k_cg_pupdate_ns_unused
#include "stpcg_kernels.inc"
#undef CG_KERNEL_ATTR
#undef CG_UPDATE_NAME
#undef CG_PUPDATE_NAME
#define CG_KERNEL_ATTR __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8)))
#define CG_UPDATE_NAME k_cg_update_ns_s80
#define CG_PUPDATE_NAME k_cg_pupdate_ns_s80_unused
#include "stpcg_kernels.inc"
#undef CG_KERNEL_ATTR
#undef CG_UPDATE_NAME
#undef CG_PUPDATE_NAME
#undef CG_UPDATE_SIGMA

// EARLY S (late r06): the direction kernel of the single-context solve without a preconditioner (v = r, plain vectors,
// G(p) by recurrence).  alpha is the A-step's -- it is in the state this kernel STARTS from -- so s += alpha p (:374)
// does not depend on this kernel's own reduction; only beta does.  Where a thread's whole walk is at most three
// elements (cfg2: two grid-stride steps + the ragged one; the host checks) every operand of the kernel is requested at
// once, behind the reduction's row loads; s is updated and stored while the other operands are still on their way;
// what is left behind the barrier is p = -v + beta p from registers.  The read phase no longer waits for the
// prologue and the prologue no longer idles the memory system (tools/microbench/stream_rates.hip: the bare stream of
// this byte mix takes 15.8 us per launch, k_cg_pupdate 18.1).  Same walk, same expressions in the same translation
// unit (same contraction), same bits as k_cg_pupdate<false, 0, NoFold>; every other form keeps that kernel.
// MEASURED (same box, alternating, rocprofv3): 17.95 us against k_cg_pupdate's 18.10, the step 55.8 against 56.1 us -- and
// with the reduction and its barrier compiled out altogether (timing build, wrong results) still 20.1-20.3 us by event
// pairs against 20.0-20.1: the prologue is NOT what separates this kernel from the bare stream (EXPERIMENTS.md r06).
// Opt-in (MI355OPT_EARLY_S=1): not the default for 0.3 us.
template <class F>
__device__ __forceinline__ void reduce_rows_1x512(const double *__restrict__ partials, int count, double &out, double *lds,
                                                  F &&after_issue) {
  // reduce_rows<1> for count <= 512: the same lane -> rows map and the same order of additions (its further eight
  // terms per lane are zeros there)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = 0.0;
  if (w == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = lane + 64 * j;
      if (r < count) t[j] = partials[r];
    }
  }
  after_issue();
  if (w == 0) {
    double v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) v += t[j];
    v = wave_reduce_sum(v);
    if (lane == 0) lds[0] = v;
  }
  __syncthreads();
  out = lds[0];
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_cg_pupdate_early(
    size_t n, CgConst cc, const CgState *__restrict__ st_in, CgState *__restrict__ st_out,
    const double *__restrict__ partials_b, int nparts_b, const double *__restrict__ v, double *__restrict__ p,
    double *__restrict__ s, HostStatus *hs, double *__restrict__ trace, size_t trace_cap, DirGramArgs dg) {
  __shared__ double lds[kWaves + 1];
  // (the walk of k_cg_pupdate, stpcg_kernels.inc, in 32-bit element indices: the host launches this kernel only where
  // n / 2 <= 3 x 512 x 1024)
  const unsigned n2 = (unsigned)(n >> 1), stride = gridDim.x * kBlock, i0 = blockIdx.x * kBlock + threadIdx.x;
  const unsigned tail0 = (unsigned)cc.rag0, per = (unsigned)cc.rag_per;
  const unsigned irem = (threadIdx.x < per) ? tail0 + blockIdx.x * per + threadIdx.x : n2;
  auto next_of = [&](unsigned i_) -> unsigned {
    const unsigned j_ = i_ + stride;
    return j_ < tail0 ? j_ : ((i_ < tail0 && irem < n2) ? irem : n2);
  };
  const unsigned ifirst = i0 < tail0 ? i0 : (irem < n2 ? irem : n2);
  unsigned Le[3];
  {
    unsigned L = ifirst;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Le[j] = L;
      if (L < n2) L = next_of(L);
    }
  }
  double2 pe[3], ve[3], se[3];
  CgState cs = load_state(st_in);
  const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
  if (cs.mode == CG_DONE) {
    if (leader) store_state(st_out, cs);
    return;
  }
  const int mode_in = cs.mode;
  auto early_s = [&] {
    if (mode_in != CG_RUN) return;
    const double alpha = cs.alpha;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (Le[j] < n2) {
        pe[j] = reinterpret_cast<double2 *>(p)[Le[j]];
        se[j] = reinterpret_cast<double2 *>(s)[Le[j]];
      }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (Le[j] < n2) ve[j] = reinterpret_cast<const double2 *>(v)[Le[j]];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (Le[j] < n2) {
        double2 sv = se[j];
        const double2 pv = pe[j];
        sv.x = sv.x + alpha * pv.x; sv.y = sv.y + alpha * pv.y;
        reinterpret_cast<double2 *>(s)[Le[j]] = sv;
      }
  };
  double red = 0;
  if (mode_in != CG_APPLY_SIGMA) reduce_rows_1x512(partials_b, nparts_b, red, lds, early_s);
  step_b(cs, cc, red);
  cs.launches = cs.launches + 1;
  if (leader) {
    store_state(st_out, cs);
    if (mode_in == CG_RUN && trace && cs.k - 1 < trace_cap) {
      const size_t k = (size_t)(cs.k - 1);
      trace[k] = cs.alpha;
      trace[trace_cap + k] = cs.beta;
      trace[2 * trace_cap + k] = cs.kappa;
      trace[3 * trace_cap + k] = cs.rv;
    }
    publish(hs, cs.launches, cs.mode == CG_DONE);
    if (dg.gdir && mode_in == CG_RUN && cs.mode == CG_RUN) {  // G(p) = -G(r) + beta G(p)  (:420)
      for (int i = 0; i < dg.ns; ++i) dg.gdir[SLOT_GDIR_P + i] = -dg.gdir[i] + cs.beta * dg.gdir[SLOT_GDIR_P + i];
    }
  }
  if (mode_in == CG_KERNEL_PENDING) {
    const double sigma = cs.sigma;
    for (unsigned i = i0; i < n2; i += stride) {
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      double2 sv = reinterpret_cast<double2 *>(s)[i];
      sv.x += sigma * pv.x; sv.y += sigma * pv.y;
      reinterpret_cast<double2 *>(s)[i] = sv;
    }
    if ((n & 1) && leader) s[n - 1] += sigma * p[n - 1];
  } else if (mode_in == CG_RUN) {
    const double alpha = cs.alpha, beta = cs.beta;
    const bool dir = cs.mode == CG_RUN;
    if (dir) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (Le[j] < n2) {
          double2 pv = pe[j];
          const double2 vv = ve[j];
          pv.x = -vv.x + beta * pv.x; pv.y = -vv.y + beta * pv.y;
          reinterpret_cast<double2 *>(p)[Le[j]] = pv;
        }
    }
    if ((n & 1) && leader) {
      s[n - 1] = s[n - 1] + alpha * p[n - 1];
      if (dir) p[n - 1] = -v[n - 1] + beta * p[n - 1];
    }
  }
}


// DEFERRED S: the direction kernel of the single-context solve in its flat form, with the step added up every SECOND
// iteration.  Nothing inside a solve reads s except the next s += alpha p (the boundary test runs on the scalar M-norm
// recurrences), so with the direction in two alternating buffers the kernel of an even iteration k leaves s alone --
//   <false>  reads v, pc = p_k;  writes px = p_k+1 = -v + beta p_k                                            [3 N]
// and the kernel of the odd iteration behind it adds both terms, in today's order and with today's roundings --
//   <true>   reads v, pc = p_k, px = p_k-1, s;  writes s = (s + alpha_k-1 p_k-1) + alpha_k p_k,
//            and px = p_k+1 = -v + beta p_k over p_k-1 (same thread, same element, read before written)       [6 N]
// 4.5 N doubles per iteration on average instead of k_cg_pupdate's 5 N.  A term is pending only while an odd iteration
// runs, and every way out of the solve adds it first:
//   * the B-step ends the solve at an even k: <false> applies s += alpha p itself (:374 is applied whatever :408-417
//     decide) and writes no direction; at an odd k <true> adds its two terms as always;
//   * boundary / negative curvature (:347-361) at an odd k: k_cg_update_ns (no s += sigma p) runs in k_cg_update's
//     place and <true> adds (s + alpha_k-1 p_k-1) + sigma p_k; at an even k k_cg_update applies it as ever;
//   * p in ker H (:305-337) at an odd k: the same with the sigma of this kernel's own B-step; at an even k as k_cg_pupdate.
// The host picks the form from its loop index, which equals the state's k for as long as the solve runs; the LAST
// enqueued iteration, when it is an even one, is k_cg_pupdate itself (nothing could be deferred to).  alpha_k-1
// travels in CgState::alpha_prev of the copy the direction kernels write (k_cg_update overwrites alpha and does not carry
// alpha_prev).  Prologue, walk and expressions are k_cg_pupdate<false, 0>'s: same translation unit, same contraction,
// same bits (tests/test_gpu_deferred_s.py).
template <bool FLUSH>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_cg_pupdate_ds(
    size_t n, CgConst cc, const CgState *__restrict__ st_in, CgState *__restrict__ st_out,
    const double *__restrict__ partials_b, int nparts_b, const double *__restrict__ v, const double *__restrict__ pc,
    double *__restrict__ px, double *__restrict__ s, HostStatus *hs, double *__restrict__ trace, size_t trace_cap,
    DirGramArgs dg) {
  __shared__ double lds[kWaves + 1];
  CgState cs = load_state(st_in);
  const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
  if (cs.mode == CG_DONE) {
    if (leader) store_state(st_out, cs);
    return;
  }
  const int mode_in = cs.mode;
  const size_t n2 = n >> 1, stride = (size_t)gridDim.x * kBlock;
  const size_t i0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  // (the walk of k_cg_pupdate, stpcg_kernels.inc: whole grid-stride steps, then the ragged rest in equal shares)
  const size_t tail0 = cc.rag0, per = cc.rag_per;
  const size_t irem = (threadIdx.x < per) ? tail0 + (size_t)blockIdx.x * per + threadIdx.x : n2;
  auto next_of = [&](size_t i_) -> size_t {
    const size_t j_ = i_ + stride;
    return j_ < tail0 ? j_ : ((i_ < tail0 && irem < n2) ? irem : n2);
  };
  const size_t ifirst = i0 < tail0 ? i0 : (irem < n2 ? irem : n2);
  double2 vv0 = make_double2(0, 0), pv0 = vv0, ov0 = vv0, sv0 = vv0;
  auto prefetch_now = [&] {
    if (ifirst < n2) {
      vv0 = reinterpret_cast<const double2 *>(v)[ifirst];
      pv0 = reinterpret_cast<const double2 *>(pc)[ifirst];
      if (FLUSH) {
        ov0 = reinterpret_cast<double2 *>(px)[ifirst];
        sv0 = reinterpret_cast<double2 *>(s)[ifirst];
      }
    }
  };
  double red[1] = {0};
  if (mode_in != CG_APPLY_SIGMA) reduce_rows<1>(partials_b, nparts_b, red, lds, prefetch_now);
  else prefetch_now();
  step_b(cs, cc, red[0]);
  cs.launches = cs.launches + 1;
  const bool dir = mode_in == CG_RUN && cs.mode == CG_RUN;
  if (leader) {
    store_state(st_out, cs);
    if (!FLUSH && dir) st_out->alpha_prev = cs.alpha;  // s += alpha p of this iteration is pending
    if (mode_in == CG_RUN && trace && cs.k - 1 < trace_cap) {
      const size_t k = (size_t)(cs.k - 1);
      trace[k] = cs.alpha;
      trace[trace_cap + k] = cs.beta;
      trace[2 * trace_cap + k] = cs.kappa;
      trace[3 * trace_cap + k] = cs.rv;
    }
    publish(hs, cs.launches, cs.mode == CG_DONE);
    if (dg.gdir && dir) {  // G(p) = -G(r) + beta G(p)  (:420)
      for (int i = 0; i < dg.ns; ++i) dg.gdir[SLOT_GDIR_P + i] = -dg.gdir[i] + cs.beta * dg.gdir[SLOT_GDIR_P + i];
    }
  }
  const double beta = cs.beta;
  if (FLUSH) {
    // the pending term, then this iteration's: alpha p (:374), or the sigma p of a boundary (:360) or kernel (:336) exit
    const double alpha_old = st_out->alpha_prev, alpha = mode_in == CG_RUN ? cs.alpha : cs.sigma;
    double2 vv = vv0, pv = pv0, ov = ov0, sv = sv0;
    for (size_t i = ifirst; i < n2;) {
      const size_t inext = next_of(i);
      double2 vn = vv, pn = pv, on = ov, sn = sv;
      if (inext < n2) {
        vn = reinterpret_cast<const double2 *>(v)[inext];
        pn = reinterpret_cast<const double2 *>(pc)[inext];
        on = reinterpret_cast<double2 *>(px)[inext];
        sn = reinterpret_cast<double2 *>(s)[inext];
      }
      sv.x = sv.x + alpha_old * ov.x; sv.y = sv.y + alpha_old * ov.y;
      sv.x = sv.x + alpha * pv.x; sv.y = sv.y + alpha * pv.y;
      reinterpret_cast<double2 *>(s)[i] = sv;
      if (dir) {
        pv.x = -vv.x + beta * pv.x; pv.y = -vv.y + beta * pv.y;
        reinterpret_cast<double2 *>(px)[i] = pv;
      }
      i = inext; vv = vn; pv = pn; ov = on; sv = sn;
    }
    if ((n & 1) && leader) {
      s[n - 1] = s[n - 1] + alpha_old * px[n - 1];
      s[n - 1] = s[n - 1] + alpha * pc[n - 1];
      if (dir) px[n - 1] = -v[n - 1] + beta * pc[n - 1];
    }
  } else if (dir) {
    double2 vv = vv0, pv = pv0;
    for (size_t i = ifirst; i < n2;) {
      const size_t inext = next_of(i);
      double2 vn = vv, pn = pv;
      if (inext < n2) {
        vn = reinterpret_cast<const double2 *>(v)[inext];
        pn = reinterpret_cast<const double2 *>(pc)[inext];
      }
      pv.x = -vv.x + beta * pv.x; pv.y = -vv.y + beta * pv.y;
      reinterpret_cast<double2 *>(px)[i] = pv;
      i = inext; vv = vn; pv = pn;
    }
    if ((n & 1) && leader) px[n - 1] = -v[n - 1] + beta * pc[n - 1];
  } else if (mode_in != CG_APPLY_SIGMA) {
    // the solve ends at this even iteration and nothing is pending: alpha p (:374), or sigma p of the kernel exit (:336)
    const double alpha = mode_in == CG_RUN ? cs.alpha : cs.sigma;
    for (size_t i = i0; i < n2; i += stride) {
      const double2 pv = reinterpret_cast<const double2 *>(pc)[i];
      double2 sv = reinterpret_cast<double2 *>(s)[i];
      sv.x = sv.x + alpha * pv.x; sv.y = sv.y + alpha * pv.y;
      reinterpret_cast<double2 *>(s)[i] = sv;
    }
    if ((n & 1) && leader) s[n - 1] = s[n - 1] + alpha * pc[n - 1];
  }
}


// ---- opt-in experiment (r05; Config::two_kernel_step) -------------------------------------------------
// ONE kernel for the A-step and the B-step of an unpreconditioned iteration over rows of Stiefel(n,3) (v == r).  Without
// a preconditioner <r+,r+> = <r,r> + 2 alpha <r,Hp> + alpha^2 <Hp,Hp> is known once the Hessian pass has also left
// <r,Hp> (k_st_hess_fused<..., TWOK>: it reads r, 8 N more bytes there), so r+ = r + alpha Hp (:377), s += alpha p (:374)
// and p+ = -r+ + beta p (:420) are one pass: reads r, Hp, p, s and writes r, p, s = 56 N bytes instead of 24 N + 40 N, and
// one kernel boundary fewer.  It CHANGES THE ROUNDING of :408 -- beta comes from a three-term recurrence that cancels
// as the residual falls, not from a sum over the new residual -- which is why it is opt-in and never the default; the
// distance from the reference it costs is measured in EXPERIMENTS.md.  The kernel test (:305-337) is served by a fifth
// extra partial, <p,r>, so every exit of STPCG is taken inside this kernel: an iteration is two launches.
template <int NS>
__global__ __launch_bounds__(kBlock) void k_cg_step2(size_t n, CgConst cc, const CgState *__restrict__ st_in,
                                                     CgState *__restrict__ st_out, const double *__restrict__ partials_a,
                                                     int nparts_a, const double *__restrict__ Hp, double *__restrict__ r,
                                                     double *__restrict__ p, double *__restrict__ s, HostStatus *hs,
                                                     double *__restrict__ trace, size_t trace_cap, DirGramArgs dg) {
  constexpr int KC = 3 + NS + 2;
  __shared__ double lds[3 * (kWaves + 1)];
  static_assert(KC <= kWaves, "one wave per component");
  CgState cs = load_state(st_in);
  const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
  if (cs.mode == CG_DONE) {
    if (leader) store_state(st_out, cs);
    return;
  }
  const size_t n2 = n >> 1, stride = (size_t)gridDim.x * kBlock, i0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  double2 hv0 = make_double2(0, 0), rv0 = hv0, pv0 = hv0, sv0 = hv0;
  auto prefetch = [&] {
    if (i0 < n2) {
      hv0 = reinterpret_cast<const double2 *>(Hp)[i0];
      rv0 = reinterpret_cast<double2 *>(r)[i0];
      pv0 = reinterpret_cast<double2 *>(p)[i0];
      sv0 = reinterpret_cast<double2 *>(s)[i0];
    }
  };
  double d[KC];
  reduce_rows<KC>(partials_a, nparts_a, d, lds, prefetch);
  step_a(cs, cc, d[0], d[1], d[2]);
  const int mode_a = cs.mode;
  double red = 0;
  {
#pragma clang fp contract(off)
    if (mode_a == CG_RUN) red = cs.rv + 2 * cs.alpha * d[KC - 2] + cs.alpha * cs.alpha * d[1];  // <r+,r+>  (:408)
    else if (mode_a == CG_KERNEL_PENDING) red = d[KC - 1];                                        // <p,r>   (:320)
  }
  step_b(cs, cc, red);
  cs.launches = cs.launches + 1;
  if (leader) {
    store_state(st_out, cs);
    if (mode_a == CG_RUN && trace && cs.k - 1 < trace_cap) {
      const size_t k = (size_t)(cs.k - 1);
      trace[k] = cs.alpha;
      trace[trace_cap + k] = cs.beta;
      trace[2 * trace_cap + k] = cs.kappa;
      trace[3 * trace_cap + k] = cs.rv;
    }
    publish(hs, cs.launches, cs.mode == CG_DONE);
    if (mode_a == CG_RUN) {
      for (int i = 0; i < NS; ++i) dg.gdir[i] = dg.gdir[i] + cs.alpha * d[3 + i];  // G(r) += alpha G(Hp)
      if (cs.mode == CG_RUN)
        for (int i = 0; i < NS; ++i) dg.gdir[SLOT_GDIR_P + i] = -dg.gdir[i] + cs.beta * dg.gdir[SLOT_GDIR_P + i];
    }
  }
  if (mode_a != CG_RUN) {  // boundary step (:359-361) or kernel step (:324-336): s += sigma p, and the solve is over
    const double sigma = cs.sigma;
    for (size_t i = i0; i < n2; i += stride) {
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      double2 sv = reinterpret_cast<double2 *>(s)[i];
      sv.x += sigma * pv.x; sv.y += sigma * pv.y;
      reinterpret_cast<double2 *>(s)[i] = sv;
    }
    if ((n & 1) && leader) s[n - 1] += sigma * p[n - 1];
    return;
  }
  const double alpha = cs.alpha, beta = cs.beta;
  const bool dir = cs.mode == CG_RUN;
  double2 hv = hv0, rv = rv0, pv = pv0, sv = sv0;
  for (size_t i = i0; i < n2;) {
    const size_t inext = i + stride;
    double2 hn = hv, rn = rv, pn = pv, sn = sv;
    if (inext < n2) {
      hn = reinterpret_cast<const double2 *>(Hp)[inext];
      rn = reinterpret_cast<double2 *>(r)[inext];
      pn = reinterpret_cast<double2 *>(p)[inext];
      sn = reinterpret_cast<double2 *>(s)[inext];
    }
    rv.x += alpha * hv.x; rv.y += alpha * hv.y;
    reinterpret_cast<double2 *>(r)[i] = rv;
    sv.x = sv.x + alpha * pv.x; sv.y = sv.y + alpha * pv.y;
    reinterpret_cast<double2 *>(s)[i] = sv;
    if (dir) {
      pv.x = -rv.x + beta * pv.x; pv.y = -rv.y + beta * pv.y;
      reinterpret_cast<double2 *>(p)[i] = pv;
    }
    i = inext; hv = hn; rv = rn; pv = pn; sv = sn;
  }
  if ((n & 1) && leader) {
    const size_t i = n - 1;
    const double rn_ = r[i] + alpha * Hp[i];
    r[i] = rn_;
    s[i] = s[i] + alpha * p[i];
    if (dir) p[i] = -rn_ + beta * p[i];
  }
}

// partial rows of sym(Y'p - (X'p) S) for the FIRST direction (p = -v, :256); later ones come from k_cg_pupdate
// (rows wider than 4 doubles, r05: 256-thread workgroups and S in LDS -- stiefel_core.h StBlk; as 1024-thread
// instantiations these two kernels spilled 250 ... 350 bytes per lane at p = 8)
template <int SP>
__global__ __launch_bounds__(StBlk<SP>::threads) void k_cg_dirgram(size_t nrows, const double *__restrict__ p, DirGramArgs dg) {
  constexpr int BLK = StBlk<SP>::threads, NW = StBlk<SP>::waves;
  constexpr bool WIDE = SP > 4;
  __shared__ double lds[SymIdx<SP>::NS * NW];
  __shared__ double SmL[WIDE ? SP * SP : 1];
  double Sm[WIDE ? 1 : SP * SP], G[SP * SP];
#pragma unroll
  for (int i = 0; i < SP * SP; ++i) G[i] = 0;
  if (WIDE) {
    if (threadIdx.x < SP * SP) SmL[threadIdx.x] = dg.S[threadIdx.x];
    __syncthreads();
  } else {
#pragma unroll
    for (int i = 0; i < SP * SP; ++i) Sm[WIDE ? 0 : i] = dg.S[i];
  }
  const size_t stride = (size_t)gridDim.x * BLK;
  for (size_t row = (size_t)blockIdx.x * BLK + threadIdx.x; row < nrows; row += stride) {
    double x[SP], y[SP], pv[SP];
#pragma unroll
    for (int c = 0; c < SP; ++c) { x[c] = dg.X[row * SP + c]; y[c] = dg.Y[row * SP + c]; pv[c] = p[row * SP + c]; }
    if (WIDE) asm volatile("" ::: "memory");
#pragma unroll
    for (int b = 0; b < SP; ++b) {
      double t = 0;
#pragma unroll
      for (int a = 0; a < SP; ++a) t += pv[a] * (WIDE ? SmL[a * SP + b] : Sm[WIDE ? 0 : a * SP + b]);
#pragma unroll
      for (int a = 0; a < SP; ++a) G[a * SP + b] += y[a] * pv[b] - x[a] * t;
    }
  }
  store_sym_partials<SP>(G, lds, dg.gpartials);
}

// the same for TWO vectors in one pass (re-anchoring, r06; rows of <= 4 doubles): partial rows of G(a) as components
// [0, NS) and of G(b) as [NS, 2 NS); X and Y are read once.  Row for row and thread for thread the sums of k_cg_dirgram.
template <int SP>
__global__ __launch_bounds__(kBlock) void k_cg_dirgram2(size_t nrows, const CgState *__restrict__ st,
                                                        const double *__restrict__ va, const double *__restrict__ vb,
                                                        DirGramArgs dg) {
  static_assert(SP >= 1 && SP <= 4, "narrow rows");
  __shared__ double lds[SymIdx<SP>::NS * kWaves];
  if (st->mode != CG_RUN) return;
  double Sm[SP * SP], Ga[SP * SP], Gb[SP * SP];
#pragma unroll
  for (int i = 0; i < SP * SP; ++i) { Ga[i] = 0; Gb[i] = 0; Sm[i] = dg.S[i]; }
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x; row < nrows; row += stride) {
    double x[SP], y[SP], a[SP], b[SP];
#pragma unroll
    for (int c = 0; c < SP; ++c) {
      x[c] = dg.X[row * SP + c]; y[c] = dg.Y[row * SP + c]; a[c] = va[row * SP + c]; b[c] = vb[row * SP + c];
    }
#pragma unroll
    for (int j = 0; j < SP; ++j) {
      double ta = 0, tb = 0;
#pragma unroll
      for (int i = 0; i < SP; ++i) { ta += a[i] * Sm[i * SP + j]; tb += b[i] * Sm[i * SP + j]; }
#pragma unroll
      for (int i = 0; i < SP; ++i) {
        Ga[i * SP + j] += y[i] * a[j] - x[i] * ta;
        Gb[i * SP + j] += y[i] * b[j] - x[i] * tb;
      }
    }
  }
  store_sym_partials<SP>(Ga, lds, dg.gpartials);
  __syncthreads();
  store_sym_partials<SP>(Gb, lds, dg.gpartials + (size_t)SymIdx<SP>::NS * kMaxRows);
}

// k_cg_init<PRE_NONE> and k_cg_dirgram in one pass for the unpreconditioned solve over rows of SP doubles (the cfg2 /
// cfg4 hot path: v = r, p = -g): g is read once, p is not read back, one launch fewer per solve (16.4 + 14.3 us as two
// kernels at cfg2).  Row r of every field belongs to the thread k_cg_dirgram gives it, so the Gram rows have its bits;
// the partial rows of <r,v> group their terms by rows instead of by pairs of elements.
template <int SP>
__global__ __launch_bounds__(StBlk<SP>::threads) void k_cg_init_dirgram(size_t nrows, const double *__restrict__ g,
                                                            double *__restrict__ r, double *__restrict__ p,
                                                            double *__restrict__ s, double *__restrict__ partials,
                                                            DirGramArgs dg) {
  constexpr int BLK = StBlk<SP>::threads, NW = StBlk<SP>::waves;
  constexpr bool WIDE = SP > 4;
  __shared__ double lds[SymIdx<SP>::NS * NW];
  __shared__ double SmL[WIDE ? SP * SP : 1];
  double Sm[WIDE ? 1 : SP * SP], G[SP * SP];
#pragma unroll
  for (int i = 0; i < SP * SP; ++i) G[i] = 0;
  if (WIDE) {
    if (threadIdx.x < SP * SP) SmL[threadIdx.x] = dg.S[threadIdx.x];
    __syncthreads();
  } else {
#pragma unroll
    for (int i = 0; i < SP * SP; ++i) Sm[WIDE ? 0 : i] = dg.S[i];
  }
  double acc[1] = {0};
  const size_t stride = (size_t)gridDim.x * BLK;
  for (size_t row = (size_t)blockIdx.x * BLK + threadIdx.x; row < nrows; row += stride) {
    double x[SP], y[SP], gv[SP], pv[SP];
#pragma unroll
    for (int c = 0; c < SP; ++c) { x[c] = dg.X[row * SP + c]; y[c] = dg.Y[row * SP + c]; gv[c] = g[row * SP + c]; }
#pragma unroll
    for (int c = 0; c < SP; ++c) {
      pv[c] = -gv[c];                      // p = -v, v = r = g  (:211,231,256)
      r[row * SP + c] = gv[c];
      s[row * SP + c] = 0 * gv[c];         // :214
      p[row * SP + c] = pv[c];
      acc[0] += gv[c] * gv[c];             // <r,v>  (:266)
    }
    if (WIDE) asm volatile("" ::: "memory");
#pragma unroll
    for (int b = 0; b < SP; ++b) {
      double t = 0;
#pragma unroll
      for (int a = 0; a < SP; ++a) t += pv[a] * (WIDE ? SmL[a * SP + b] : Sm[WIDE ? 0 : a * SP + b]);
#pragma unroll
      for (int a = 0; a < SP; ++a) G[a * SP + b] += y[a] * pv[b] - x[a] * t;
    }
  }
  store_sym_partials<SP>(G, lds, dg.gpartials);
  __syncthreads();
  block_partials_store_w<1, NW>(acc, lds, partials);
}

// recurrence form: G(p0) from the rows k_cg_dirgram left (or the all-reduced slots); G(r0) = -G(p0) (p0 = -r0)
__global__ __launch_bounds__(kBlock) void k_cg_gdir_init(const double *__restrict__ partials, int count, int ns,
                                                         const double *__restrict__ slots, int from_slots,
                                                         double *__restrict__ gdir) {
  if (!from_slots) {
    gdir_from_rows(partials, count, ns, gdir);
    return;
  }
  if (threadIdx.x < ns) {
    const double v = slots[threadIdx.x];
    gdir[SLOT_GDIR_P + threadIdx.x] = v;
    gdir[threadIdx.x] = -v;
  }
}

// Re-anchoring of the recurrence form (r06): dst = G(vector) from the rows k_cg_dirgram just left (or the all-reduced
// slots).  The recurrences G(r') = G(r) + alpha G(Hp), G(p') = -G(r') + beta G(p) carry an ABSOLUTE error of the size
// rounding had at the scale of the residual they started from; on identical inputs a 200-iteration solve ends 2.6e-13
// from the reference with them and 8e-15 with the two-pass operator, and follows the reference's alpha trace for 354
// instead of 395 iterations (tests/test_gpu_long_solves.py).  Every mi_ctx::cfg.reanchor iterations both are replaced
// by their direct values.  A solve that has left CG_RUN keeps what it has (its kernels do nothing any more).
// dst2 != nullptr: components [ns, 2 ns) go there (the two-vector pass k_cg_dirgram2)
__global__ __launch_bounds__(kBlock) void k_cg_gdir_anchor(const double *__restrict__ partials, int count, int ns,
                                                           const double *__restrict__ slots, int from_slots,
                                                           const CgState *__restrict__ st, double *__restrict__ dst,
                                                           double *__restrict__ dst2) {
  if (st->mode != CG_RUN) return;
  if (!from_slots) {
    gdir_rows_to(partials, count, ns, dst);
    if (dst2) gdir_rows_to(partials + (size_t)ns * kMaxRows, count, ns, dst2);
    return;
  }
  if (threadIdx.x < ns) dst[threadIdx.x] = slots[threadIdx.x];
  if (dst2 && threadIdx.x < ns) dst2[threadIdx.x] = slots[ns + threadIdx.x];
}

// OBSERVED SOLVE (mi_stpcg_observed): the reference's user function (IterativeSolvers.h:50-59) is called once per pass
// after alpha_k is known and the boundary tests have passed, before any update (:365-369).  In the fused step that is
// the moment between the operator pass and k_cg_update: s += alpha p of the LAST pass has been applied (it lives in the
// direction kernel), nothing of THIS pass has, and alpha_k with every branch decision of :300-362 follows from the
// three curvature sums the operator left as partial rows.  k_cg_peek tells the host: ONE workgroup re-reduces components
// 0..2 of those rows with the consumers' own reduce_rows (component by component, fixed order: the consumers' totals bit
// for bit, whatever else their rows carry), runs step_a on a COPY of the live state and stores
//   {mode on entry, mode after step_a, alpha, k}
// into pinned host words, the context's polled flag behind them.  The live state is not written: k_cg_update repeats
// step_a from the same rows as in every other solve -- its instantiations, and the un-observed solve, are untouched.
__global__ __launch_bounds__(kBlock) void k_cg_peek(CgConst cc, const CgState *__restrict__ st,
                                                    const double *__restrict__ partials_a, int nparts_a,
                                                    unsigned long long *host, unsigned long long *flag,
                                                    unsigned long long seq) {
  __shared__ double lds[3 * (kWaves + 1)];
  CgState cs = load_state(st);
  const int mode_in = cs.mode;
  if (mode_in == CG_RUN) {  // (the same in every thread: the barriers of the reduction are uniform)
    double d[3];
    reduce_rows<3>(partials_a, nparts_a, d, lds);
    step_a(cs, cc, d[0], d[1], d[2]);
  }
  if (threadIdx.x != 0) return;
  host[0] = (unsigned long long)mode_in;
  host[1] = (unsigned long long)cs.mode;
  reinterpret_cast<double *>(host)[2] = cs.alpha;
  host[3] = cs.k;
  __threadfence_system();
  if (flag) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the observer said stop: the reference's `break` at :369 -- |s|_M from the recurrence (:424), k completed updates, and
// nothing of this pass in s, r or p.  One thread, in place: no kernel of the solve is in flight beside it.
__global__ void k_cg_user_stop(CgState *st, HostStatus *hs) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  CgState cs = load_state(st);
  if (cs.mode != CG_RUN) return;
  cs.M_norm = sqrt(cs.sk_M_2);  // :424
  cs.exit_reason = MI_STPCG_EXIT_USER;
  cs.mode = CG_DONE;
  store_state(st, cs);
  publish(hs, cs.launches, 1);
}

inline void cpu_relax() { __builtin_ia32_pause(); }

}  // namespace

namespace mi {
int launch_dot3_partials(mi_ctx *ctx, size_t n, const double *x, const double *y, int *nparts) {
  const int grid = grid_for(ctx, n, 4);
  KScope ks(ctx, MI_K_CG_DOT3);
  hipLaunchKernelGGL(k_cg_dot3, dim3(grid), dim3(kBlock), 0, ctx->stream, n, ctx->cg_live, x, y,
                     ctx->partials);
  *nparts = grid;
  return MI_OK;
}
}  // namespace mi

extern "C" {

void mi_stpcg_default_params(mi_stpcg_params *p) {
  if (!p) return;
  p->Delta = 1.0;
  p->max_iterations = 1000;  // :172
  p->kappa_fgr = .1;
  p->theta = .5;
  p->epsilon = 1e-8;  // :179
  p->run_ahead = 0;  // 0: the library default (3, or MI355OPT_RUN_AHEAD)
  p->constraint_At = 0;
  p->defer_result = 0;
}

// the sticky failure word of the solve's preconditioner (mi_precon::fail_word) travels right behind the state copy
static inline double *precon_fail_host(mi_ctx *ctx) { return reinterpret_cast<double *>(ctx->cg_host + 1); }
// Code 1 (the preconditioner's inner iteration BROKE DOWN: p'Sp <= 0, NaN / Inf) is an error of the solve: its result is
// not a projected step.  Code 2 (the inner iteration stopped at its iteration limit short of its tolerance) is NOT: a
// caller that caps inner_max_iterations to bound the cost asks for an inexact projection -- the solve
// returns MI_OK, mi_stpcg_result::precon_status says 2, and mi_precon_constraint_info has the residual that was left.
static int precon_fail_check(mi_ctx *ctx, mi_stpcg_result *result) {
  const double w = *precon_fail_host(ctx);
  if (result) result->precon_status = (int)w;
  if (w != 1.0) return MI_OK;
  set_error("the preconditioner of this solve reported a failed application (code 1: its inner iteration broke down -- "
            "dependent constraint rows, or NaN / Inf in the residual): the result is not a projected step");
  return MI_ERR_INTERNAL;
}

// The final state of a solve lands in the pinned words by a kernel store, the polled sequence number behind it
// (context.hip: stream_wait): no copy engine and no wake-up between a solve and its caller.
__global__ void k_cg_result_to_host(unsigned long long *host, const unsigned long long *__restrict__ st,
                                    const double *__restrict__ fail_dev, unsigned long long *flag,
                                    unsigned long long seq) {
  constexpr int kWords = (int)(sizeof(CgState) / 8);
  static_assert(sizeof(CgState) % 8 == 0, "CgState is copied in 8-byte words");
  if (threadIdx.x < kWords) host[threadIdx.x] = st[threadIdx.x];
  if (threadIdx.x == kWords) reinterpret_cast<double *>(host)[kWords] = fail_dev ? *fail_dev : 0.0;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// enqueue that kernel; returns the sequence number to poll for, 0 when polling is off (the caller copies instead)
static unsigned long long result_to_host(mi_ctx *ctx, const CgState *st_final, const mi_precon *P) {
  unsigned long long *flag = nullptr, *hdev = nullptr;
  unsigned long long seq = poll_begin(ctx, &flag);
  if (!seq) return 0;
  if (hipHostGetDevicePointer((void **)&hdev, ctx->cg_host, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;  // (the sequence number stays unused: the next one is larger)
  }
  hipLaunchKernelGGL(k_cg_result_to_host, dim3(1), dim3(64), 0, ctx->stream, hdev,
                     reinterpret_cast<const unsigned long long *>(st_final),
                     (const double *)(P ? P->fail_word : nullptr), flag, seq);
  if (hipGetLastError() != hipSuccess) return 0;  // (nothing was enqueued: the caller copies)
  return seq;
}

}  // extern "C"

// ---- host driver of the fused solve: a plan (what to launch), an owner of the work vectors, a function per step ----
namespace {

// Dispatch on the compile-time parameters of the solve's kernels, in the shape of DISPATCH_P (mi_internal.h): the
// statement runs with NAME as a compile-time constant, one of four values (the last one: every other x)
#define DISPATCH_4(x, NAME, A, B, C, D, ...)                \
  switch (x) {                                              \
    case A: { constexpr int NAME = A; __VA_ARGS__; } break; \
    case B: { constexpr int NAME = B; __VA_ARGS__; } break; \
    case C: { constexpr int NAME = C; __VA_ARGS__; } break; \
    default: { constexpr int NAME = D; __VA_ARGS__; } break; \
  }
#define DISPATCH_PRE(pre, ...) DISPATCH_4(pre, PRE, PRE_NONE, PRE_DIAG, PRE_BLOCK3, PRE_EXTERNAL, __VA_ARGS__)
// components of the operator's partial rows in the recurrence form (dir_comps), p = 1 ... 4
#define DISPATCH_KC(kc, ...) DISPATCH_4(kc, KC, 4, 6, 9, 16, __VA_ARGS__)
// p = 5 ... 8: 18, 24, 31, 39 components (3 + p (p + 1) / 2).  Never folded (the host keeps the separate exchange for
// them), and launched from the uncapped kernel: 39 reduced values per thread do not fit the 64 vector registers the
// two-workgroups-per-CU twins are held to
#define DISPATCH_KC_WIDE(kc, ...) DISPATCH_4(kc, KC, 18, 24, 31, 39, __VA_ARGS__)
// row width of the direction kernel (0: flat form)
#define DISPATCH_SP(sp, ...) \
  if ((sp) == 0) { constexpr int SP = 0; __VA_ARGS__; } else DISPATCH_4(sp, SP, 1, 2, 3, 4, __VA_ARGS__)

// Which inclusion of stpcg_kernels.inc a single-rank launch takes (`if constexpr`: only the chosen kernel is
// instantiated).  Recurrence form, 4 / 6 / 9 components: k_cg_update (SIGMA) or k_cg_update_ns; 16 components always need
// the 80-SGPR twin (see above).
template <bool SIGMA, int KC>
auto cg_update_recur_kernel() {
  if constexpr (SIGMA && KC == 16) return &k_cg_update_s80<PRE_NONE, false, KC, NoFold>;
  else if constexpr (SIGMA) return &k_cg_update<PRE_NONE, false, KC, NoFold>;
  else if constexpr (KC == 16) return &k_cg_update_ns_s80<PRE_NONE, false, KC, NoFold>;
  else return &k_cg_update_ns<PRE_NONE, false, KC, NoFold>;
}
// (rows of 0 / 1 doubles are the two forms that count on 8 waves per SIMD -- the twin wherever the plain kernel is
// allocated more than 80 scalar registers: rows of 1, and the slot-reading flat form; wider rows are bound by their
// vector registers)
template <bool FS, int SP>
auto cg_pupdate_kernel() {
  if constexpr (SP == 1 || (FS && SP == 0)) return &k_cg_pupdate_s80<FS, SP, NoFold>;
  else return &k_cg_pupdate<FS, SP, NoFold>;
}

// What one solve launches.  Filled ONCE by stpcg_plan, before anything is allocated or enqueued, and const from there on:
// every enqueue step reads its decisions here and takes none of its own.  (Each field's rule: stpcg_plan.)
struct StpcgPlan {
  size_t n;
  bool observed, sharded, rows, lockstep, recur, folded, init_fused, gdir_in_scalar_init;
  bool twok, early, defer;  // forms of the step, mutually exclusive (none of them: the plain three-kernel step)
  int pre, run_ahead, grid, gns, sp, kc, reanchor;
  const mi_dirgram *dgp;
  CgConst cc;
};

int stpcg_plan(const mi_ctx *ctx, const mi_op *H, const mi_precon *P, const mi_stpcg_params *prm, size_t n,
               bool observed, StpcgPlan &pl) {
  pl.n = n;
  pl.observed = observed;
  pl.pre = !P ? PRE_NONE : (P->kind == 1 ? PRE_DIAG : (P->kind == 2 ? PRE_BLOCK3 : PRE_EXTERNAL));
  MI_REQUIRE(pl.pre != PRE_BLOCK3 || n % 3 == 0, "block-Jacobi preconditioner needs n divisible by 3");
  // several ranks: the partial rows themselves are all-reduced (rows_mode) and the consumers keep
  // their prologue re-reduction; the slot variants stay reachable through MI355OPT_FORCE_SLOT_PATH
  pl.sharded = slot_mode(ctx);
  pl.rows = rows_mode(ctx);
  // direction-Gram fusion (mi_op::dirgram): one-pass Hessian, the Gram rows come from the direction kernel
  pl.dgp = (!ctx->no_dirgram && H->dirgram && H->apply_dir) ? H->dirgram : nullptr;
  // rows wider than 4 doubles (Stiefel p = 5 ... 8) have the one-pass operator in its recurrence form only (no
  // preconditioner); with one, the operator keeps its two passes and the direction kernel its flat form
  if (pl.dgp && pl.dgp->p > 4 && (pl.pre != PRE_NONE || ctx->dirgram_direct)) pl.dgp = nullptr;
  MI_REQUIRE(!pl.dgp || (pl.dgp->p >= 1 && pl.dgp->p <= kMaxP && pl.dgp->n * (size_t)pl.dgp->p == n),
             "operator's direction-Gram description does not match the problem dimension");
  // (default depth 3: depth 2 gives the same cfg2 step and -0.6 % on a cfg3 TNT run)
  pl.run_ahead = prm->run_ahead > 0 ? prm->run_ahead : 3;
  pl.lockstep = (ctx->comm != nullptr && ctx->world_size > 1) || ctx->force_lockstep;
  pl.grid = (pl.pre == PRE_BLOCK3) ? grid_for(ctx, n / 3, 2) : grid_for(ctx, n, 4);
  pl.cc = CgConst{prm->Delta, prm->Delta * prm->Delta, prm->epsilon, (unsigned long long)prm->max_iterations, 0ull, 0ull};
  const size_t n2 = n >> 1, step = (size_t)pl.grid * kBlock;
  pl.cc.rag0 = (n2 / step) * step;
  pl.cc.rag_per = (n2 - pl.cc.rag0 + (size_t)pl.grid - 1) / (size_t)pl.grid;
  // recurrence form of the direction Gram: needs v == r (no preconditioner)
  pl.recur = pl.dgp && pl.pre == PRE_NONE && !ctx->dirgram_direct;
  pl.gns = pl.dgp ? pl.dgp->p * (pl.dgp->p + 1) / 2 : 0;
  pl.sp = (pl.dgp && !pl.recur) ? pl.dgp->p : 0;  // row form of k_cg_pupdate only in the direct form
  pl.kc = pl.recur ? dir_comps(pl.dgp->p) : 3;    // components of the operator's partial rows
  // Several ranks through the peer-memory layer, unpreconditioned recurrence form (the cfg2 / cfg4 hot loop): the two
  // scalar exchanges of an iteration are folded into the prologues of their consumers (no exchange kernels).  Every
  // other combination keeps the separate exchange kernels.
  // (the folded exchange carries at most kIpcVals = 16 values: p <= 4)
  pl.folded = pl.sharded && pl.recur && pl.kc <= kIpcVals && comm_fold_enabled(ctx) && !ctx->force_slot_path;
  // unpreconditioned recurrence form: initialisation and the first direction's Gram rows in one pass
  // (k_cg_init_dirgram); one rank, nothing to exchange: G(p0), G(r0) set by k_cg_scalar_init itself
  pl.init_fused = pl.recur && n == pl.dgp->n * (size_t)pl.dgp->p;
  pl.gdir_in_scalar_init = pl.recur && !pl.sharded && !pl.rows;
  // opt-in experiment: the two-kernel step (k_cg_step2; one rank, Stiefel(n,3) in the window form)
  // (an observed solve keeps the plain three-kernel step: the two-kernel step has no point between the operator and
  // the update, the early-s form is an experiment, and the deferred-s form would show the observer of an odd pass an s
  // that is one term short)
  pl.twok = ctx->cfg.two_kernel_step && pl.recur && pl.dgp->twok && pl.dgp->p == 3 && !pl.sharded && !pl.rows &&
            !pl.lockstep && pl.init_fused && pl.gdir_in_scalar_init && !observed;
  // (the early-s form: single context, v = r or any plain vector, at most three elements per thread, <= 512 rows)
  pl.early = !pl.sharded && !pl.rows && pl.sp == 0 && ctx->cfg.early_s && pl.grid <= 512 &&
             pl.cc.rag0 <= 2ull * (size_t)pl.grid * kBlock && (n >> 1) < ((size_t)1 << 31) && !observed;
  // deferred-s form (k_cg_pupdate_ds): single context, flat direction kernel; the direction lives in two buffers that
  // swap every iteration -- StpcgBufs::p is the current one wherever a step names it
  pl.defer = !pl.sharded && !pl.rows && !pl.lockstep && !pl.twok && pl.sp == 0 && !pl.early && ctx->cfg.defer_s &&
             !observed;
  // r06: re-anchor the recurrence form's G(p), G(r) by the direct form every `reanchor` iterations, 0: never (the count is
  // the loop index: the same on every rank, so the exchanges it carries stay matched across ranks)
  pl.reanchor = (pl.recur && !pl.twok && ctx->cfg.reanchor > 0) ? ctx->cfg.reanchor : 0;
  return MI_OK;
}

// What the enqueue steps work on: the solve's work vectors (pool vectors), which it owns, and the buffers that are fixed
// for the solve.  Its destructor is the ONE way out of a solve once it exists: a `return` anywhere behind it can neither
// leak the vectors nor leave the context marked as inside a solve.  Only p / p2 change inside the loop (the deferred-s
// form's swap, stpcg_bstep): every step reads them here, so the swap reaches all later ones.
struct StpcgBufs {
  mi_ctx *ctx;
  mi_vec *r = nullptr, *v = nullptr, *p = nullptr, *p2 = nullptr, *Hp = nullptr;
  bool ok = false;  // set on the successful exit only
  const mi_vec *g = nullptr; mi_vec *s_out = nullptr; mi_op *H = nullptr;
  mi_precon *P = nullptr; const mi_stpcg_params *prm = nullptr;
  double *vd = nullptr;          // v aliases r when P is absent (:231,383)
  const double *pred = nullptr;  // data of the built-in preconditioners
  DirGramArgs dga{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  double *slots_g = nullptr, *slots_a = nullptr, *slots_b = nullptr;  // (slots_g: the recurrence form's, kc <= 16 doubles)
  CgState *st0 = nullptr, *st1 = nullptr;
  double *tr = nullptr;          // device trace (4 rows of tcap doubles), or null
  size_t tcap = 0;
  // r'-halo form (Config::halo_rprime): the halo rows of r' travel with the <r,v> all-reduce, halo(p') is formed locally
  bool rprime = false;
  unsigned long long *peek_dev = nullptr;  // observed solve: device address of the pinned words
  explicit StpcgBufs(mi_ctx *c) : ctx(c) {}
  StpcgBufs(const StpcgBufs &) = delete;
  StpcgBufs &operator=(const StpcgBufs &) = delete;
  ~StpcgBufs() {
    ctx->cg_live = nullptr;
    // a folded halo push nobody consumed must not outlive the solve on ANY exit: p is a recycled pool pointer, and the
    // next solve's first Hessian pass would match the stale (A, p, V) entry, skip the real exchange and wait for a flag
    // that never comes (r04, ADVICE: an error exit between comm_halo_fold_next and the pass used to leave it set)
    comm_halo_fold_drop(ctx);
    // (an error exit: what was enqueued may still be reading the vectors that go back to the pool)
    if (!ok) (void)hipStreamSynchronize(ctx->stream);
    for (mi_vec *x : {r, p, p2, Hp, v}) mi_vec_destroy(x);  // (null: nothing to do)
  }
};

int stpcg_bufs(mi_ctx *ctx, const StpcgPlan &pl, const mi_vec *g, mi_op *H, mi_precon *P, const mi_stpcg_params *prm,
               mi_vec *s_out, const mi_stpcg_trace *trace, StpcgBufs &b) {
  const size_t n = pl.n;
  b.g = g, b.s_out = s_out, b.H = H, b.P = P, b.prm = prm;
  MI_TRY(mi_vec_create(ctx, n, &b.r));
  MI_TRY(mi_vec_create(ctx, n, &b.p));
  MI_TRY(mi_vec_create(ctx, n, &b.Hp));
  if (pl.pre != PRE_NONE) MI_TRY(mi_vec_create(ctx, n, &b.v));
  if (pl.defer) MI_TRY(mi_vec_create(ctx, n, &b.p2));
  b.vd = (pl.pre == PRE_NONE) ? b.r->d : b.v->d;
  b.pred = P ? P->data : nullptr;
  if (trace && trace->cap) {
    if (ctx->trace_cap < trace->cap) {
      if (ctx->trace_dev) MI_HIP(hipFree(ctx->trace_dev));
      MI_HIP(hipMalloc((void **)&ctx->trace_dev, 4 * trace->cap * sizeof(double)));
      ctx->trace_cap = trace->cap;
    }
    b.tcap = ctx->trace_cap;  // layout stride
    b.tr = ctx->trace_dev;
  }
  if (pl.dgp)
    b.dga = DirGramArgs{pl.dgp->X, pl.dgp->Y, pl.dgp->S, ctx->partials2, pl.recur ? ctx->scalars + SLOT_GDIR : nullptr,
                        pl.gns};
  b.slots_g = ctx->scalars + SLOT_GRAM, b.slots_a = ctx->scalars + SLOT_CG, b.slots_b = ctx->scalars + SLOT_CG + 4;
  b.st0 = ctx->cg, b.st1 = ctx->cg1;
  // observed solve: k_cg_peek's four words land at the head of the pinned state copy (free until the final read-back)
  if (pl.observed) {
    const hipError_t e = hipHostGetDevicePointer((void **)&b.peek_dev, ctx->cg_host, 0);
    if (e != hipSuccess) return hip_fail(e, "stpcg observer: device address of the pinned words", __FILE__, __LINE__);
  }
  return MI_OK;
}

// completes the sum of k components of `count` partial rows across the ranks (one rank: nothing to do)
int stpcg_allreduce(mi_ctx *ctx, const StpcgPlan &pl, double *partials, int count, int k, double *slots) {
  return pl.sharded ? reduce_rows_allreduce(ctx, partials, count, k, slots)
                    : pl.rows ? comm_allreduce_rows(ctx, partials, k) : MI_OK;
}

// ---- the argument list of each kernel family, once ----
int launch_dirgram(mi_ctx *ctx, const StpcgPlan &pl, const StpcgBufs &b, const double *vec) {
  DISPATCH_P(pl.dgp->p, hipLaunchKernelGGL(k_cg_dirgram<P>, dim3(pl.grid), dim3(StBlk<P>::threads), 0, ctx->stream,
                                           pl.dgp->n, vec, b.dga));
  return MI_OK;
}
void launch_gdir_anchor(mi_ctx *ctx, const StpcgPlan &pl, const StpcgBufs &b, double *dst, double *dst2) {
  hipLaunchKernelGGL(k_cg_gdir_anchor, dim3(1), dim3(kBlock), 0, ctx->stream, (const double *)ctx->partials2, pl.grid,
                     pl.gns, (const double *)b.slots_g, pl.sharded ? 1 : 0, (const CgState *)b.st0, dst, dst2);
}
template <class K, class FOLD>
void launch_cg_update(K kernel, mi_ctx *ctx, const StpcgPlan &pl, const StpcgBufs &b, int nparts, const FOLD &fold) {
  hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(kBlock), 0, ctx->stream, pl.n, pl.cc, (const CgState *)b.st0, b.st1,
                     (const double *)ctx->partials, nparts, (const double *)(pl.recur ? b.slots_g : b.slots_a),
                     (const double *)b.p->d, (const double *)b.Hp->d, b.pred, b.s_out->d, b.r->d, b.vd, ctx->partials_b,
                     b.dga, fold);
}
template <class K, class FOLD>
void launch_cg_pupdate(K kernel, mi_ctx *ctx, const StpcgPlan &pl, const StpcgBufs &b, const FOLD &fold) {
  hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(kBlock), 0, ctx->stream, pl.n, pl.cc, (const CgState *)b.st1, b.st0,
                     (const double *)ctx->partials_b, pl.grid, (const double *)b.slots_b, (const double *)b.vd, b.p->d,
                     b.s_out->d, ctx->status_dev, b.tr, b.tcap, b.dga, fold);
}

// ---- enqueue steps ----------------------------------------------------------------------------
// v = P(r) by the preconditioner's own kernels, then the partial rows of <r,v> (`first`: in the set-up, and p = -v)
int stpcg_precondition(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b, bool first) {
  mi_precon *P = b.P;
  if (P->apply_project) MI_TRY(P->apply_project(P, b.r, b.v, b.prm->constraint_At));  // (v, lambda) = P(r); r -= A' lambda (:386,403)
  else MI_TRY(P->apply(P, b.r, b.v));                                                 // v = P(r) (:386)
  hipLaunchKernelGGL(first ? &k_cg_dot_rv<true> : &k_cg_dot_rv<false>, dim3(pl.grid), dim3(kBlock), 0, ctx->stream, pl.n,
                     (const CgState *)(first ? b.st0 : b.st1), (const double *)b.r->d, (const double *)b.v->d, b.p->d,
                     ctx->partials_b);
  return MI_OK;
}

// set-up: initialisation, the first direction's Gram rows, scalar init
int stpcg_setup(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b) {
  hipStream_t st = ctx->stream;
  const int grid = pl.grid;
  {
    KScope ks(ctx, MI_K_CG_INIT);
    if (pl.init_fused) {
      DISPATCH_P(pl.dgp->p, hipLaunchKernelGGL(k_cg_init_dirgram<P>, dim3(grid), dim3(StBlk<P>::threads), 0, st, pl.dgp->n,
                                               (const double *)b.g->d, b.r->d, b.p->d, b.s_out->d, ctx->partials_b, b.dga));
    } else {
      DISPATCH_PRE(pl.pre, hipLaunchKernelGGL(k_cg_init<PRE>, dim3(grid), dim3(kBlock), 0, st, pl.n, (const double *)b.g->d,
                                              b.pred, b.r->d, b.vd, b.p->d, b.s_out->d, ctx->partials_b));
    }
  }
  if (pl.pre == PRE_EXTERNAL) MI_TRY(stpcg_precondition(ctx, pl, b, true));
  if (pl.dgp) {
    if (!pl.init_fused) MI_TRY(launch_dirgram(ctx, pl, b, b.p->d));
    if (pl.recur && !pl.gdir_in_scalar_init) {
      MI_TRY(stpcg_allreduce(ctx, pl, ctx->partials2, grid, pl.gns, b.slots_g));
      hipLaunchKernelGGL(k_cg_gdir_init, dim3(1), dim3(kBlock), 0, st, (const double *)ctx->partials2, grid, pl.gns,
                         (const double *)b.slots_g, pl.sharded ? 1 : 0, b.dga.gdir);
    }
  }
  const CgSetup cfg{b.prm->Delta, b.prm->kappa_fgr, b.prm->theta, b.prm->epsilon,
                    (unsigned long long)b.prm->max_iterations};
  MI_TRY(stpcg_allreduce(ctx, pl, ctx->partials_b, grid, 1, b.slots_b));
  if (pl.sharded)
    hipLaunchKernelGGL(k_cg_scalar_init<true>, dim3(1), dim3(kBlock), 0, st, b.st0, cfg, (const double *)ctx->partials_b,
                       grid, (const double *)b.slots_b, ctx->status_dev, (const double *)nullptr, 0, 0, (double *)nullptr);
  else
    hipLaunchKernelGGL(k_cg_scalar_init<false>, dim3(1), dim3(kBlock), 0, st, b.st0, cfg, (const double *)ctx->partials_b,
                       grid, (const double *)b.slots_b, ctx->status_dev, (const double *)ctx->partials2, grid, pl.gns,
                       pl.gdir_in_scalar_init ? b.dga.gdir : (double *)nullptr);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "stpcg init launch", __FILE__, __LINE__);
  return MI_OK;
}

// re-anchor (StpcgPlan::reanchor): G(p), G(r) of the recurrence form, formed afresh by the direct form
int stpcg_reanchor(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b) {
  const int grid = pl.grid, gns = pl.gns;
  if (pl.dgp->p <= 4) {
    // rows of <= 4 doubles: both Grams from ONE pass over X, Y, p, r and one (all-)reduction of 2 gns components
    DISPATCH_P4(pl.dgp->p, hipLaunchKernelGGL(k_cg_dirgram2<P>, dim3(grid), dim3(kBlock), 0, ctx->stream, pl.dgp->n,
                                              (const CgState *)b.st0, (const double *)b.p->d, (const double *)b.r->d, b.dga));
    MI_TRY(stpcg_allreduce(ctx, pl, ctx->partials2, grid, 2 * gns, b.slots_g));
    launch_gdir_anchor(ctx, pl, b, b.dga.gdir + SLOT_GDIR_P, b.dga.gdir);
  } else {
    for (int which = 0; which < 2; ++which) {
      MI_TRY(launch_dirgram(ctx, pl, b, which == 0 ? b.p->d : b.r->d));
      MI_TRY(stpcg_allreduce(ctx, pl, ctx->partials2, grid, gns, b.slots_g));
      launch_gdir_anchor(ctx, pl, b, b.dga.gdir + (which == 0 ? SLOT_GDIR_P : 0), nullptr);
    }
  }
  return MI_OK;
}

// operator pass: Hp = H(p) (:294) + partial rows of <p,Hp>, <Hp,Hp>, <p,p> in ctx->partials
int stpcg_operator(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b, int *nparts) {
  if (pl.dgp) return b.H->apply_dir(b.H, b.p, b.Hp, pl.recur ? -1 : pl.grid, nparts);
  if (b.H->apply_dots) return b.H->apply_dots(b.H, b.p, b.Hp, nparts);
  MI_TRY(b.H->apply(b.H, b.p, b.Hp));
  return launch_dot3_partials(ctx, pl.n, b.p->d, b.Hp->d, nparts);
}

// the whole iteration of the two-kernel step (StpcgPlan::twok): two launches; the state ping-pongs between st0 and st1
// ACROSS iterations, *st_final is the copy this one wrote
int stpcg_step2(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b, size_t k, CgState **st_final) {
  CgState *cur = (k & 1) ? b.st1 : b.st0, *nxt = (k & 1) ? b.st0 : b.st1;
  int nparts = 0;
  ctx->cg_live = cur;
  ctx->twok_r = b.r->d;
  const int st_op = b.H->apply_dir(b.H, b.p, b.Hp, -2, &nparts);
  ctx->twok_r = nullptr;
  MI_TRY(st_op);
  KScope ks(ctx, MI_K_CG_UPDATE);
  hipLaunchKernelGGL(k_cg_step2<6>, dim3(pl.grid), dim3(kBlock), 0, ctx->stream, pl.n, pl.cc, (const CgState *)cur, nxt,
                     (const double *)ctx->partials, nparts, (const double *)b.Hp->d, b.r->d, b.p->d, b.s_out->d,
                     ctx->status_dev, b.tr, b.tcap, b.dga);
  *st_final = nxt;
  return MI_OK;
}

// Observed solve, between the operator pass and the A-step: alpha_k and the decisions of :300-362 to the host (one small
// kernel and one polled wait per pass), then the user's function.
// *says: go on; enqueue nothing more; or enqueue the rest of this pass, which ends the solve (no further peek)
enum ObserverSays { OBS_GO_ON, OBS_STOP, OBS_LAST_PASS };
int stpcg_observe(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b, mi_stpcg_observer observer, void *observer_user,
                  int nparts, ObserverSays *says) {
  hipStream_t st = ctx->stream;
  ctx->host_syncs++;
  unsigned long long *flag = nullptr;
  const unsigned long long seq = poll_begin(ctx, &flag);
  {
    KScope ks(ctx, MI_K_CG_SCALAR_A);
    hipLaunchKernelGGL(k_cg_peek, dim3(1), dim3(kBlock), 0, st, pl.cc, (const CgState *)b.st0,
                       (const double *)ctx->partials, nparts, b.peek_dev, seq ? flag : (unsigned long long *)nullptr, seq);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "stpcg observer peek launch", __FILE__, __LINE__);
  MI_TRY(poll_finish(ctx, seq, "stpcg observer peek"));
  const volatile unsigned long long *pk = reinterpret_cast<const volatile unsigned long long *>(ctx->cg_host);
  const int mode_in = (int)pk[0], mode_a = (int)pk[1];
  *says = OBS_STOP;
  // (this pass's operator is already enqueued -- hvp_calls counts ENQUEUED passes, here as in the un-observed solve --
  // unless the test of the status word at the top of the loop happened to see the exit first)
  if (mode_in == CG_DONE) return MI_OK;  // the last pass's B-step (or the initialisation) ended the solve: :285, :290
  if (mode_a != CG_RUN) {
    *says = OBS_LAST_PASS;  // kernel-of-H or boundary exit inside this pass: the reference does not call either
    return MI_OK;
  }
  double alpha_k;
  const unsigned long long abits = pk[2];
  memcpy(&alpha_k, &abits, sizeof(alpha_k));
  ctx->cg_in_observer = true;
  const int stop = observer(observer_user, (size_t)pk[3], b.s_out, b.r, b.v ? b.v : b.r, b.p, alpha_k);
  ctx->cg_in_observer = false;
  *says = stop ? OBS_STOP : OBS_GO_ON;
  if (!stop) return MI_OK;
  hipLaunchKernelGGL(k_cg_user_stop, dim3(1), dim3(64), 0, st, b.st0, ctx->status_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "stpcg observer stop launch", __FILE__, __LINE__);
  return MI_OK;
}

// A-step (k_cg_update*): the operator's partial rows complete across the ranks, then the update
int stpcg_astep(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b, size_t k, int nparts) {
  // (deferred-s form, odd k: a term of s is pending, and a boundary step is the direction kernel's to apply behind it)
  const bool sigma_later = pl.defer && (k & 1);
  // recurrence form: 3 dots + the Gram rows of Hp in one reduction (and one exchange across ranks)
  FoldArgs fold_a;
  // folded: the sum over the ranks completes in the kernel's own prologue (comm_ipc.h): no exchange kernel
  if (pl.folded) fold_a = comm_fold_next(ctx);
  else MI_TRY(stpcg_allreduce(ctx, pl, ctx->partials, nparts, pl.kc, pl.recur ? b.slots_g : b.slots_a));
  KScope ks(ctx, MI_K_CG_UPDATE);
  // (every kernel named here is launched by some form of the solve: the choice inside a dispatch adds no instantiation)
  if (!pl.recur) {
    DISPATCH_PRE(pl.pre, launch_cg_update(pl.sharded    ? &k_cg_update<PRE, true, 3, NoFold>
                                          : sigma_later ? &k_cg_update_ns<PRE, false, 3, NoFold>
                                                        : &k_cg_update<PRE, false, 3, NoFold>,
                                          ctx, pl, b, nparts, NoFold{}));
  } else if (pl.kc > 16) {
    DISPATCH_KC_WIDE(pl.kc, launch_cg_update(pl.sharded    ? &k_cg_update<PRE_NONE, true, KC, NoFold>
                                             : sigma_later ? &k_cg_update_ns<PRE_NONE, false, KC, NoFold>
                                                           : &k_cg_update<PRE_NONE, false, KC, NoFold>,
                                             ctx, pl, b, nparts, NoFold{}));
  } else if (pl.folded) {
    DISPATCH_KC(pl.kc, launch_cg_update(&k_cg_update_s80<PRE_NONE, false, KC, FoldArgs>, ctx, pl, b, nparts, fold_a));
  } else {
    DISPATCH_KC(pl.kc, launch_cg_update(pl.sharded    ? &k_cg_update_s80<PRE_NONE, true, KC, NoFold>
                                        : sigma_later ? cg_update_recur_kernel<false, KC>()
                                                      : cg_update_recur_kernel<true, KC>(),
                                        ctx, pl, b, nparts, NoFold{}));
  }
  return MI_OK;
}

// B-step (k_cg_pupdate*): the partial rows of <r,v> complete across the ranks, then the new direction (with the r'-halo
// tail).  The deferred-s form swaps p and p2 here.
int stpcg_bstep(mi_ctx *ctx, const StpcgPlan &pl, StpcgBufs &b, size_t k) {
  hipStream_t st = ctx->stream;
  const mi_dirgram *dgp = pl.dgp;
  const int grid = pl.grid;
  if (pl.folded) {
    const FoldArgs fold_b = comm_fold_next(ctx);  // (folded <=> recurrence form <=> sp == 0)
    // ... and the halo exchange of the NEXT Hessian pass rides in this kernel's stores of the new direction
    FoldPush fp{fold_b, HaloPush{}};
    const bool push = dgp->halo_A && k + 1 < b.prm->max_iterations &&
                      comm_halo_fold_next(ctx, dgp->halo_A, dgp->p, b.p->d, &fp.h);
    KScope ks(ctx, MI_K_CG_PUPDATE);
    if (push) launch_cg_pupdate(&k_cg_pupdate_s80<false, 0, FoldPush>, ctx, pl, b, fp);
    else launch_cg_pupdate(&k_cg_pupdate_s80<false, 0, FoldArgs>, ctx, pl, b, fold_b);
  } else if (pl.sharded) {
    MI_TRY(reduce_rows_allreduce(ctx, ctx->partials_b, grid, 1, b.slots_b));
    if (b.rprime) MI_TRY(comm_rprime_exchange(ctx, dgp->halo_A, dgp->p, b.r->d, nullptr, 0));
    KScope ks(ctx, MI_K_CG_PUPDATE);
    DISPATCH_SP(pl.sp, launch_cg_pupdate(cg_pupdate_kernel<true, SP>(), ctx, pl, b, NoFold{}));
  } else {
    if (pl.rows && b.rprime) MI_TRY(comm_rprime_exchange(ctx, dgp->halo_A, dgp->p, b.r->d, ctx->partials_b, 1));
    else if (pl.rows) MI_TRY(comm_allreduce_rows(ctx, ctx->partials_b, 1));
    KScope ks(ctx, MI_K_CG_PUPDATE);
    if (pl.early) {
      hipLaunchKernelGGL(k_cg_pupdate_early, dim3(grid), dim3(kBlock), 0, st, pl.n, pl.cc, (const CgState *)b.st1, b.st0,
                         (const double *)ctx->partials_b, grid, (const double *)b.vd, b.p->d, b.s_out->d, ctx->status_dev,
                         b.tr, b.tcap, b.dga);
    } else if (pl.defer && ((k & 1) || k + 1 < b.prm->max_iterations)) {
      // odd k: the pending term and this one (FLUSH); even k: this one stays pending
      hipLaunchKernelGGL((k & 1) ? &k_cg_pupdate_ds<true> : &k_cg_pupdate_ds<false>, dim3(grid), dim3(kBlock), 0, st,
                         pl.n, pl.cc, (const CgState *)b.st1, b.st0, (const double *)ctx->partials_b, grid,
                         (const double *)b.vd, (const double *)b.p->d, b.p2->d, b.s_out->d, ctx->status_dev, b.tr,
                         b.tcap, b.dga);
      std::swap(b.p, b.p2);
    } else {  // (deferred-s form: the last enqueued iteration is an even one)
      DISPATCH_SP(pl.sp, launch_cg_pupdate(cg_pupdate_kernel<false, SP>(), ctx, pl, b, NoFold{}));
    }
  }
  if (b.rprime && (pl.sharded || pl.rows)) {
    const double *hr = nullptr;
    double *hp = nullptr;
    size_t cnt = 0;
    comm_rprime_buffers(ctx, dgp->halo_A, dgp->p, &hr, &hp, &cnt);
    if (cnt) {
      const int hg = (int)std::max<size_t>(1, std::min<size_t>((cnt + 255) / 256, 512));
      hipLaunchKernelGGL(k_halo_dir, dim3(hg), dim3(256), 0, st, (const CgState *)b.st0, hr, hp, cnt);
    }
    comm_rprime_mark(ctx, dgp->halo_A, dgp->p, b.p->d);
  }
  return MI_OK;
}

// the pinned copy of the final state -> the caller's result (mi_stpcg and mi_stpcg_collect; hvp_calls is theirs)
int stpcg_result_from_host(mi_ctx *ctx, mi_stpcg_result *result) {
  int ipc_err = 0;
  (void)mi_comm_ipc_error(ctx, &ipc_err);
  if (ipc_err) {
    set_error("a wait in the peer-memory exchange layer timed out: the result of this solve is invalid");
    return MI_ERR_COMM;
  }
  const CgState &f = *ctx->cg_host;
  result->update_step_M_norm = f.M_norm;
  result->num_iterations = (size_t)f.k;
  result->exit_reason = f.exit_reason;
  result->rv_final = f.rv;
  return precon_fail_check(ctx, result);
}

// read-back of the final state: deferred (the copy travels behind the solve; whoever waits for the stream next, or
// mi_stpcg_collect, completes it), or here
int stpcg_readback(mi_ctx *ctx, const StpcgPlan &pl, const StpcgBufs &b, const CgState *st_final, mi_stpcg_trace *trace,
                   mi_stpcg_result *result) {
  hipStream_t st = ctx->stream;
  const mi_precon *P = b.P;
  const bool tracing = trace && trace->cap;
  *precon_fail_host(ctx) = 0.0;
  if (b.prm->defer_result && !tracing && !pl.observed) {
    hipError_t e = hipSuccess;
    ctx->cg_deferred_seq = result_to_host(ctx, st_final, P);
    if (!ctx->cg_deferred_seq) {
      if (!ctx->cg_deferred_ev) e = hipEventCreateWithFlags(&ctx->cg_deferred_ev, hipEventDisableTiming);
      if (e == hipSuccess) e = hipMemcpyAsync(ctx->cg_host, st_final, sizeof(CgState), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && P && P->fail_word)
        e = hipMemcpyAsync(precon_fail_host(ctx), P->fail_word, sizeof(double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipEventRecord(ctx->cg_deferred_ev, st);
    }
    if (e != hipSuccess) return hip_fail(e, "stpcg deferred read-back", __FILE__, __LINE__);
    ctx->cg_deferred = true;
    ctx->cg_deferred_hvp = result->hvp_calls;
    result->update_step_M_norm = result->rv_final = 0;
    result->num_iterations = 0, result->exit_reason = -1, result->precon_status = 0;
    return MI_OK;
  }
  ctx->host_syncs++;
  if (const unsigned long long seq = result_to_host(ctx, st_final, P)) {
    MI_TRY(poll_finish(ctx, seq, "stpcg read-back"));
  } else {
    hipError_t e = hipMemcpyAsync(ctx->cg_host, st_final, sizeof(CgState), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && P && P->fail_word)
      e = hipMemcpyAsync(precon_fail_host(ctx), P->fail_word, sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "stpcg read-back", __FILE__, __LINE__);
  }
  MI_TRY(stpcg_result_from_host(ctx, result));
  if (tracing) {
    const size_t len = result->num_iterations < trace->cap ? result->num_iterations : trace->cap;
    trace->len = len;
    double *dst[4] = {trace->alpha, trace->beta, trace->kappa, trace->rv};
    for (int c = 0; c < 4; ++c)
      if (dst[c] && len) {
        const hipError_t e = hipMemcpy(dst[c], ctx->trace_dev + (size_t)c * b.tcap, len * sizeof(double),
                                       hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "stpcg trace copy", __FILE__, __LINE__);
      }
  }
  return MI_OK;
}

// mi_stpcg (observer == nullptr) and mi_stpcg_observed share this body; the plan's `observed` is false for the former,
// which enqueues exactly what it always did
int stpcg_solve(mi_ctx *ctx, const mi_vec *g, mi_op *H, mi_precon *P, const mi_stpcg_params *prm,
                mi_stpcg_observer observer, void *observer_user, mi_vec *s_out, mi_stpcg_result *result,
                mi_stpcg_trace *trace) {
  MI_REQUIRE(ctx && g && H && prm && s_out && result, "null argument");
  MI_REQUIRE(g->ctx == ctx && s_out->ctx == ctx && H->ctx == ctx, "objects belong to another context");
  MI_REQUIRE(g->n == s_out->n && g->n == H->n, "dimension mismatch: g %zu, s %zu, H %zu", g->n,
             s_out->n, H->n);
  MI_REQUIRE(g->d != s_out->d, "g and s_out must not alias");
  MI_REQUIRE(!ctx->cg_in_observer, "a solve was started on this context from inside an STPCG observer");
  const bool observed = observer != nullptr;
  if (observed) {
    // nothing has been touched or counted yet: the caller keeps its own loop
    const char *why = nullptr;
    if (mi_stpcg_observer_available(ctx, &why) != MI_OK) {
      set_error("mi_stpcg_observed declined: %s", why);
      return MI_DECLINED;
    }
  }
  touch(s_out);
  ctx->fusion.fused_stpcg_solves++;
  MI_REQUIRE(!P || (P->ctx == ctx && P->n == g->n), "preconditioner dimension/context mismatch");
  MI_REQUIRE(!prm->constraint_At || (P && P->apply_project),
             "constraint_At needs a constraint preconditioner (mi_precon_create_constraint)");
  MI_REQUIRE(!(P && P->kind == 3 && ctx->world_size > 1),
             "the constraint preconditioner is single-rank: its reductions are not completed across ranks");
  // reference argument checks, IterativeSolvers.h:183-205
  MI_REQUIRE(prm->Delta > 0, "Trust-region radius (Delta) must be a positive real value");
  MI_REQUIRE(prm->kappa_fgr >= 0 && prm->kappa_fgr < 1,
             "Target fractional reduction of the gradient norm (kappa_fgr) must be a real value in "
             "the range [0,1)");
  MI_REQUIRE(prm->theta >= 0 && prm->theta <= 1,
             "Target superlinear convergence rate (theta) must be a real value in the range [0,1]");
  MI_REQUIRE(prm->epsilon > 0 && prm->epsilon < 1,
             "Relative norm tolerance for declaring a vector to lie in the kernel of H (epsilon) "
             "should be a small positive number in the range (0,1)");

  RangeScope range("mi_stpcg");
  comm_halo_fold_drop(ctx);  // (nothing may be pending from an earlier solve: see ~StpcgBufs)
  StpcgPlan plan;
  MI_TRY(stpcg_plan(ctx, H, P, prm, g->n, observed, plan));
  const StpcgPlan &pl = plan;
  StpcgBufs b(ctx);
  // (allocates the residual-halo buffers on first use; a rank that cannot must fail HERE, loudly, rather than take
  // another collective sequence than its peers -- ADVICE r05)
  if (pl.recur && !pl.folded && pl.dgp->halo_A) MI_TRY(comm_rprime_prepare(ctx, pl.dgp->halo_A, &b.rprime));
  // the failure word is per solve: a NaN residual in one solve must not condemn the object for the next
  if (P && P->fail_word) MI_HIP(hipMemsetAsync(P->fail_word, 0, sizeof(double), ctx->stream));
  MI_TRY(stpcg_bufs(ctx, pl, g, H, P, prm, s_out, trace, b));
  ctx->cg_deferred = false;  // (a result nobody collected is superseded)
  ctx->cg_deferred_seq = 0;
  ctx->epoch++;
  ctx->status->word = 0;
  ctx->status->epoch = ctx->epoch;
  ctx->cg_live = b.st0;
  MI_TRY(stpcg_setup(ctx, pl, b));

  // --- main loop: speculative enqueue with bounded run-ahead -----------------------------------
  CgState *st_final = b.st0;
  size_t hvp = 0;
  for (size_t k = 0; k < prm->max_iterations; ++k) {
    // throttle: at most run_ahead launches ahead of the device
    uint64_t w = ctx->status->word;
    while (!observed && !(w & 1) && k > (w >> 1) + (uint64_t)pl.run_ahead) {  // (an observed solve never runs ahead)
      cpu_relax();
      w = ctx->status->word;
    }
    if (w & 1) {
      // One rank: stop as soon as the exit is seen.  Several ranks: every enqueued iteration carries
      // collectives, so all ranks must enqueue the SAME number -- exactly (launches at exit) + run_ahead,
      // a function of the replicated device state only, not of when this host happened to look.  (No
      // rank can get past that count unknowingly: the throttle holds it until the exit is published.)
      if (!pl.lockstep || k >= (w >> 1) + (uint64_t)pl.run_ahead) break;
    }
    if (pl.reanchor && k > 0 && k % (size_t)pl.reanchor == 0) MI_TRY(stpcg_reanchor(ctx, pl, b));
    if (pl.twok) {
      MI_TRY(stpcg_step2(ctx, pl, b, k, &st_final));
      ++hvp;
      continue;
    }
    int nparts = 0;
    MI_TRY(stpcg_operator(ctx, pl, b, &nparts));
    ++hvp;
    ObserverSays says = OBS_GO_ON;
    if (observed) MI_TRY(stpcg_observe(ctx, pl, b, observer, observer_user, nparts, &says));
    if (says == OBS_STOP) break;
    MI_TRY(stpcg_astep(ctx, pl, b, k, nparts));
    if (pl.pre == PRE_EXTERNAL) MI_TRY(stpcg_precondition(ctx, pl, b, false));
    MI_TRY(stpcg_bstep(ctx, pl, b, k));
    if (says == OBS_LAST_PASS) break;
  }
  result->hvp_calls = hvp;
  comm_halo_fold_drop(ctx);  // (a push behind the last enqueued iteration has no reader)
  MI_TRY(stpcg_readback(ctx, pl, b, st_final, trace, result));
  b.ok = true;  // (no synchronisation on this exit)
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_stpcg_collect(mi_ctx *ctx, mi_stpcg_result *result) {
  MI_REQUIRE(ctx && result, "null argument");
  MI_REQUIRE(ctx->cg_deferred, "mi_stpcg_collect: no deferred solve is pending on this context");
  ctx->cg_deferred = false;
  if (ctx->cg_deferred_seq) {
    const unsigned long long seq = ctx->cg_deferred_seq;
    ctx->cg_deferred_seq = 0;
    if (__atomic_load_n(ctx->poll_flag, __ATOMIC_ACQUIRE) < seq) {
      ctx->host_syncs++;
      MI_TRY(poll_finish(ctx, seq, "stpcg deferred read-back"));
    }
  } else {
    hipError_t e = hipEventQuery(ctx->cg_deferred_ev);
    if (e == hipErrorNotReady) {
      e = hipEventSynchronize(ctx->cg_deferred_ev);
      ctx->host_syncs++;
    }
    if (e != hipSuccess) return hip_fail(e, "stpcg deferred read-back", __FILE__, __LINE__);
  }
  result->hvp_calls = ctx->cg_deferred_hvp;
  return stpcg_result_from_host(ctx, result);
}

int mi_stpcg_observer_available(mi_ctx *ctx, const char **why) {
  MI_REQUIRE(ctx, "null argument");
  const char *w = nullptr;  // (literals: they outlive the call)
  if (ctx->cfg.no_fused_observer) w = "MI355OPT_NO_FUSED_OBSERVER is set";
  else if (ctx->world_size > 1) w = "the context is one of several ranks";
  else if (ctx->force_lockstep) w = "MI355OPT_FORCE_LOCKSTEP is set";
  else if (slot_mode(ctx) || rows_mode(ctx)) w = "the context completes its reductions through an exchange layer";
  if (why) *why = w ? w : "";
  return w ? MI_DECLINED : MI_OK;
}

int mi_stpcg(mi_ctx *ctx, const mi_vec *g, mi_op *H, mi_precon *P, const mi_stpcg_params *prm, mi_vec *s_out,
             mi_stpcg_result *result, mi_stpcg_trace *trace) {
  return stpcg_solve(ctx, g, H, P, prm, nullptr, nullptr, s_out, result, trace);
}

int mi_stpcg_observed(mi_ctx *ctx, const mi_vec *g, mi_op *H, mi_precon *P, const mi_stpcg_params *prm,
                      mi_stpcg_observer fn, void *user, mi_vec *s_out, mi_stpcg_result *result, mi_stpcg_trace *trace) {
  MI_REQUIRE(fn, "mi_stpcg_observed: null observer (mi_stpcg is the solve without one)");
  return stpcg_solve(ctx, g, H, P, prm, fn, user, s_out, result, trace);
}

}  // extern "C"
