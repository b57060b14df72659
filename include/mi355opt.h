/* mi355opt.h -- C ABI of libmi355opt.so: the MI355X (gfx950) device layer underneath the
 * Optimization::Riemannian::TNT / Optimization::LinearAlgebra::STPCG / LOBPCG function templates.
 *
 * The reference (david-m-rosen/Optimization) is a header-only C++ template library with no FFI:
 * its "interface" for this path is the implicit Vector concept (operators used at
 * LinearAlgebra/IterativeSolvers.h:211-420, Riemannian/TNT.h:375-557) plus user-supplied
 * std::function callables (Riemannian/Concepts.h:44-112).  This header is what a C++ maintainer
 * binds underneath those templates: every entry point below names the
 * reference expression(s) it realises on the device.  File:line citations are relative to
 * /root/reference/include/Optimization.
 *
 * Conventions
 *   - plain C, opaque handles, no C++/torch types; every function returns an mi_status (0 = ok);
 *     mi_last_error() gives the message of the calling thread's last failure.
 *   - all work is enqueued on the context's HIP stream and is asynchronous unless documented as
 *     synchronous ("sync").  One context = one GPU = one stream; not thread-safe per context (the
 *     reference is single-threaded).
 *   - vectors are flat fp64 arrays in HBM.  A Stiefel / Euclidean n x p matrix is row-major
 *     (p contiguous), SO(3)^N variables are N row-major 3x3 blocks, so(3)^N tangents are 3N doubles.
 *   - there is NO CPU fallback: without a GPU every compute entry point fails with
 *     MI_ERR_NO_DEVICE.
 */
#ifndef MI355OPT_H
#define MI355OPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_API __attribute__((visibility("default")))

typedef enum mi_status {
  MI_OK = 0,
  MI_ERR_INVALID_ARGUMENT = 1, /* the checks the reference answers with std::invalid_argument */
  MI_ERR_HIP = 2,
  MI_ERR_OOM = 3,
  MI_ERR_NO_DEVICE = 4,
  MI_ERR_COMM = 5,
  MI_ERR_INTERNAL = 6,
  MI_DECLINED = 7 /* not an error: the entry point does not take this call on the context as it is configured; nothing was
                     done or counted, mi_last_error() names the cause, the caller keeps its own path (mi_stpcg_observed) */
} mi_status;

typedef struct mi_ctx mi_ctx;       /* device context: stream, memory pool, scalar file, communicator */
typedef struct mi_vec mi_vec;       /* fp64 device vector */
typedef struct mi_csr mi_csr;       /* sparse matrix (CSR on input, sliced-ELL-64 in HBM) */
typedef struct mi_bsr3 mi_bsr3;     /* 3x3-block sparse matrix (pose-graph Hessians) */
typedef struct mi_op mi_op;         /* symmetric linear operator on tangent vectors (the HVP) */
typedef struct mi_precon mi_precon; /* preconditioner v = M^-1 r */
typedef struct mi_stiefel_rq mi_stiefel_rq; /* Rayleigh-quotient problem on St(n,p) */
typedef struct mi_so3n mi_so3n;             /* chordal rotation-averaging problem on SO(3)^N */

/* ---------------------------------------------------------------------------------------------
 * (1) context / stream / pool
 * ------------------------------------------------------------------------------------------- */
MI_API const char *mi_version(void);
MI_API const char *mi_last_error(void);
MI_API const char *mi_status_string(int status);
MI_API int mi_device_count(int *count);
MI_API int mi_ctx_create(int device, mi_ctx **out);
MI_API int mi_ctx_destroy(mi_ctx *ctx);
MI_API int mi_ctx_sync(mi_ctx *ctx);                   /* sync: hipStreamSynchronize */
/* number of times the library waited for the device on this context (scalar read-backs, solver exits, explicit
 * syncs; uploads/downloads of whole vectors not counted): how often the host sits on the critical path of e.g. one
 * TNT outer iteration (tools/bench_tnt.py) */
MI_API int mi_ctx_sync_count(mi_ctx *ctx, size_t *count);
/* Which side of the fusion boundary the work of this context ran on (r06).  The template layer selects the fused
 * entry points by probing its std::function arguments with target<>() (Riemannian/TNT.h, LinearAlgebra/
 * IterativeSolvers.h of this repository): a client that wraps a tagged callable in a lambda of its own -- a logger, a
 * penalty term, the adapter style of the reference's own TNT.h:400-426 -- silently gets the generic loop (one host
 * synchronisation per inner product).  These counters make that visible: the fused_* fields count calls of the fused
 * entry points (mi_stpcg, mi_lsqr, mi_*_trial), generic_inner_products counts host-synchronising inner products
 * (mi_vec_dot, mi_vec_dot_batch), and the generic_* solver fields are reported by the template layer through
 * mi_ctx_note_generic when a solve on MI355::DeviceVector falls to its generic loop.  With MI355OPT_WARN_GENERIC=1 in the
 * environment the first such fall of each kind also prints one line on stderr saying which probe failed. */
typedef struct mi_fusion_counters {
  unsigned long long fused_stpcg_solves;
  unsigned long long generic_stpcg_solves;
  unsigned long long fused_lsqr_solves;
  unsigned long long generic_lsqr_solves;
  unsigned long long fused_trial_steps;      /* TNT / GradientDescent trial points evaluated by one fused chain */
  unsigned long long generic_trial_steps;    /* ... by the reference's statement sequence on DeviceVector */
  unsigned long long generic_inner_products; /* host-synchronising inner products */
} mi_fusion_counters;
enum { MI_GENERIC_STPCG = 0, MI_GENERIC_LSQR = 1, MI_GENERIC_TRIAL = 2 };
MI_API int mi_ctx_fusion_counters(mi_ctx *ctx, mi_fusion_counters *out);
MI_API int mi_ctx_fusion_counters_reset(mi_ctx *ctx);
/* template layer -> library: a solve / trial step of kind `what` (MI_GENERIC_*) on device vectors ran the generic loop;
 * `why` (may be NULL) names the probe that failed */
MI_API int mi_ctx_note_generic(mi_ctx *ctx, int what, const char *why);
MI_API int mi_ctx_stream(mi_ctx *ctx, void **stream);  /* the hipStream_t all work is enqueued on */
MI_API int mi_ctx_device_name(mi_ctx *ctx, char *buf, size_t buflen);
MI_API int mi_ctx_pool_bytes(mi_ctx *ctx, size_t *bytes_reserved);

/* HIP-event timing of whole regions and of individual kernels (bench.py's roofline leg).
 * Kernel ids are the MI_K_* values; when timing is enabled for an id every launch of that kernel is
 * bracketed by an event pair on the context stream. */
enum {
  MI_K_NONE = 0,
  MI_K_CG_INIT, MI_K_CG_DOT3, MI_K_CG_SCALAR_A, MI_K_CG_UPDATE, MI_K_CG_SCALAR_B, MI_K_CG_PUPDATE,
  MI_K_SPMM, MI_K_STIEFEL_SPMM_GRAM, MI_K_STIEFEL_GRAM_REDUCE, MI_K_STIEFEL_FINISH_DOTS,
  MI_K_STIEFEL_RETRACT, MI_K_BSR3_SPMV_DOTS, MI_K_BLAS1, MI_K_LOBPCG_GRAM, MI_K_LOBPCG_UPDATE,
  MI_K_LOBPCG_RESIDUAL, MI_K_STIEFEL_HESS_FUSED,
  MI_K_COMM_ALLREDUCE, /* a scalar exchange across ranks that is a launch of its own: one RCCL all-reduce (group) or
                          one exchange kernel of the peer-memory layer; folded exchanges have none */
  MI_K_COMM_HALO,      /* a halo exchange that is a launch of its own: ncclSend/ncclRecv group or push kernel */
  MI_K_SO3_GRAD,        /* the gradient-only assembly pass of mi_so3n_gradient / mi_so3n_armijo_trial */
  MI_K_SO3_RESIDUAL,    /* k_so3_residual: F(R) of mi_so3n_residual */
  MI_K_SO3_JAC,         /* k_so3_jac: dF xi over the edges (apply and apply_sub_scaled forms) */
  MI_K_SO3_JACT,        /* k_so3_jact: dF* y over the incidences (apply and apply_sub_scaled forms) */
  MI_K_SO3_EDGE_WEIGHT, /* k_so3_edge_weight: the per-edge pass of mi_so3n_reweight */
  MI_K_SO3_INC_REWEIGHT, /* k_so3_inc_reweight: the per-incidence pass of mi_so3n_reweight */
  MI_K_PGO_MODEL,       /* k_pgo_model in its model form: the assembly pass of mi_pgo_model */
  MI_K_PGO_GRAD,        /* k_pgo_model in its other forms: mi_pgo_objective, mi_pgo_gradient, the trial chain */
  MI_K_PGO_HVP,         /* k_pgo_hvp: the joint Hessian-vector product (with and without the curvature dots) */
  MI_K_PGO_RETRACT,     /* k_pgo_retract */
  MI_K_COUNT
};
/* The library's switches (A/B forms of its kernels, verification hooks of the multi-rank path) are read from the
 * environment ONCE per context, in mi_ctx_create: MI355OPT_<NAME>=<integer> for NAME in FORCE_SLOT_PATH,
 * FORCE_LOCKSTEP, FORCE_UNIFORM_GRID, MAX_GRID, NO_DIRGRAM, DIRGRAM_DIRECT, IPC_TIMEOUT_MS, NO_FOLD, HALO_PUSH_LATE,
 * NO_PACKED, NO_WINDOW, NO_WIN_BOUNDS, NO_FAR_COMPUTED, WORDS16, NO_SPMM_STREAM, NO_SPMM_WIN, NO_UPDATE_MFMA,
 * NO_ZERO_COPY, NO_GRAM_HALF, NO_UPDATE_PAIR, SO3_NO_QUAT, SO3_NO_RQUAT, SO3_SORT_NBR, HALO_RPRIME, TWO_KERNEL_STEP, WIDE_QUAD,
 * NO_POLLED_SYNC, WARN_GENERIC, REANCHOR, NO_SPMM_SWEEP, SWEEP_ZSEGS, WIDE_WINDOW, EARLY_S, DEFER_S, NO_FUSED_OBSERVER (DESIGN.md / INTEGRATION.md say what each selects).  For the boolean switches a value that
 * is not an integer counts as 1 unless it is "no" / "false" / "off"; the integer-valued ones (MAX_GRID, IPC_TIMEOUT_MS,
 * WIDE_QUAD, WIDE_WINDOW, SO3_SORT_NBR, REANCHOR, SWEEP_ZSEGS) take integers only -- anything else is ignored with a warning and the default stays.
 * WORDS16 is ON by default (the one-pass Stiefel Hessian streams a matrix with at most 32 table values as 16-bit
 * window words: same bits, fewer bytes); WORDS16=0 keeps the 4-byte words, and it takes integers only as well.  A
 * context with TWO_KERNEL_STEP set keeps the 4-byte words whatever WORDS16 says.  Any other
 * MI355OPT_* variable found in the environment (a removed or misspelt switch) gets one warning on stderr.  mi_ctx_set_option changes one on a live context (name with or without the MI355OPT_
 * prefix); format switches (NO_PACKED) act when a matrix is created, the communication ones before the layer they
 * concern is brought up.  Nothing else in the library reads the environment. */
MI_API int mi_ctx_set_option(mi_ctx *ctx, const char *name, long value);
MI_API int mi_ktime_enable(mi_ctx *ctx, int kernel_id, int on);
MI_API int mi_ktime_reset(mi_ctx *ctx);
/* sync: resolves recorded event pairs; returns launches and total milliseconds for kernel_id */
MI_API int mi_ktime_read(mi_ctx *ctx, int kernel_id, size_t *launches, double *total_ms);
MI_API const char *mi_kernel_name(int kernel_id);
/* Profiler ranges (SURVEY.md 8(b) group 9): roctx markers, visible to `rocprofv3 --marker-trace`.  The library
 * brackets its own solves (mi_stpcg, mi_lsqr) with ranges of those names; callers may nest their own (e.g. one per
 * TNT outer iteration, TNT.h:436-683).  No-ops (still MI_OK) when no ROCTx library (rocprofiler-sdk-roctx, else roctracer's libroctx64) is installed. */
MI_API int mi_range_push(const char *name);
MI_API int mi_range_pop(void);
MI_API int mi_timer_start(mi_ctx *ctx);             /* records an event on the stream */
MI_API int mi_timer_stop(mi_ctx *ctx, double *ms);  /* sync: records, waits, returns elapsed ms */

/* ---------------------------------------------------------------------------------------------
 * (2) vectors -- the implicit Vector concept
 * ------------------------------------------------------------------------------------------- */
MI_API int mi_vec_create(mi_ctx *ctx, size_t n, mi_vec **out); /* `Vector v;` + sizing; pooled */
MI_API int mi_vec_destroy(mi_vec *v);                           /* returns storage to the pool */
/* non-owning window [offset, offset+n) of `base` (e.g. a column block of a column-major panel:
 * `S.leftCols(ns)`, `S.middleCols(..)` LOBPCG.h:254-268); destroy with mi_vec_destroy.  Destruction order is free:
 * an owner destroyed while views of it are alive keeps its storage until the last view is destroyed (a handle to the
 * destroyed owner itself must of course not be used again). */
MI_API int mi_vec_view(const mi_vec *base, size_t offset, size_t n, mi_vec **out);
MI_API int mi_vec_len(const mi_vec *v, size_t *n);
MI_API int mi_vec_data(const mi_vec *v, void **device_ptr);
/* Announce a write made OUTSIDE the library through the pointer of mi_vec_data (torch interop, a user kernel): problem
 * objects cache speculative results keyed on a vector's contents (the trial point of mi_stiefel_rq_trial /
 * mi_so3n_trial), and every library entry point that writes a vector advances its generation stamp itself -- a view
 * shares the stamp of the vector that owns the storage -- but a raw-pointer write is invisible to it. */
MI_API int mi_vec_touch(mi_vec *v);
MI_API int mi_vec_upload(mi_vec *v, const double *host, size_t n);         /* sync */
MI_API int mi_vec_download(const mi_vec *v, double *host, size_t n);       /* sync */
MI_API int mi_vec_copy(mi_vec *dst, const mi_vec *src);   /* `r_k = g;` IterativeSolvers.h:214,231,383 */
MI_API int mi_vec_fill(mi_vec *v, double a);
MI_API int mi_vec_scale(mi_vec *v, double a);             /* `p_k *= -1;` :324 ; `u /= beta` :653 */
MI_API int mi_vec_div(mi_vec *v, double a);               /* `u /= beta` :653,712, `v /= alpha` :658,723: a true
                                                             division, rounded like the reference's */
MI_API int mi_vec_scale_to(mi_vec *z, double a, const mi_vec *x); /* z = a * x: `0 * g` :211 (0 * Inf = NaN, -0.0
                                                             kept), `sigma_k * p_k`, unary minus :256 */
MI_API int mi_vec_axpy(mi_vec *y, double a, const mi_vec *x); /* `s_k += sigma_k * p_k;` :336,360,377 */
/* z = a*x + b*y (z may alias x or y): `s_k = s_k + alpha_k*p_k` :374, `p_k = -v_k + beta_k*p_k` :420,
 * `0 * g` :211, unary minus :256, `X + V` Riemannian/Concepts.h:189 */
MI_API int mi_vec_axpby(mi_vec *z, double a, const mi_vec *x, double b, const mi_vec *y);
/* sync: `V1.dot(V2)` Riemannian/Concepts.h:178 -- deterministic two-stage reduction */
MI_API int mi_vec_dot(const mi_vec *x, const mi_vec *y, double *out);
/* k <= 4 inner products in one pass, results to host (sync) */
MI_API int mi_vec_dot_batch(mi_ctx *ctx, int k, const mi_vec *const *x, const mi_vec *const *y,
                            double *out);

/* ---------------------------------------------------------------------------------------------
 * (3) sparse operators (user HVP building blocks; the reference has none -- its HVP is a user
 *     callable invoked at IterativeSolvers.h:294 and TNT.h:512)
 * ------------------------------------------------------------------------------------------- */
MI_API int mi_csr_create(mi_ctx *ctx, size_t n, size_t nnz, const int32_t *rowptr,
                         const int32_t *col, const double *val, mi_csr **out); /* sync (upload) */
MI_API int mi_csr_destroy(mi_csr *A);
/* W (n x p row-major) = A V ; 1 <= p <= 16 (p = 9 ... 16: one context, not row-sharded) */
MI_API int mi_csr_spmm(const mi_csr *A, int p, const mi_vec *V, mi_vec *W);

/* ---------------------------------------------------------------------------------------------
 * (4) linear operators and preconditioners handed to STPCG
 *     mi_op     <-> SymmetricLinearOperator<Vector> H   (LinearAlgebra/Concepts.h:20-21; called at
 *                   IterativeSolvers.h:294)
 *     mi_precon <-> STPCGPreconditioner<Vector,Multiplier> P with Multiplier = nullptr_t
 *                   (IterativeSolvers.h:83-85; called at :234,386; TNT.h:413-419)
 * ------------------------------------------------------------------------------------------- */
/* callback: must ENQUEUE out = Op(in) on the context stream and return MI_OK without synchronising */
typedef int (*mi_apply_fn)(void *user, const mi_vec *in, mi_vec *out);
MI_API int mi_op_create_callback(mi_ctx *ctx, size_t n, mi_apply_fn fn, void *user, mi_op **out);
/* rectangular operator (n_in -> n_out), e.g. a Jacobian and its adjoint for LSQR / TNLS */
MI_API int mi_op_create_callback_rect(mi_ctx *ctx, size_t n_in, size_t n_out, mi_apply_fn fn, void *user,
                                      mi_op **out);
/* A USER operator with the solver's reductions inside its own pass (r04).  The whole point of the reference is the
 * user-supplied Hessian (`H(p)` at IterativeSolvers.h:294, bound from the caller's QuadraticModel at TNT.h:400-426); a
 * plain callback operator pays a separate 2N-byte pass for the three curvature inner products of :300,305-306.  A
 * fused callback leaves them behind itself, like the built-in operators do: next to out = Op(in) the user's kernel
 * writes, for each of its workgroups b in [0, rows), the workgroup's partial sums of
 *     component 0: <in, out>     component 1: <out, out>     component 2: <in, in>
 * at args->partials[c * args->partial_stride + b] (fp64, EVERY row in [0, rows) written, zeros for idle workgroups) and
 * reports `rows`.  Contract: 1 <= rows <= args->max_rows; if args->required_rows > 0 (several ranks with RCCL: every
 * rank must leave the same number of rows) rows must equal it; the partial sums must be deterministic (fixed-order
 * reduction inside the workgroup, no atomics) because every workgroup of the consuming kernel re-reduces the rows in a
 * fixed order and all of them must obtain the same bits.  Everything is enqueued on args->stream (the context's
 * stream), nothing may synchronise.  With such an operator a fused STPCG iteration is three launches for ANY HIP
 * operator: the user's pass, k_cg_update, k_cg_pupdate.  `fn` is the same product without the sums (mi_op_apply, the
 * `dm` product of TNT.h:512).  examples/stpcg_user_stencil.hip is a complete client. */
typedef struct mi_fused_args {
  double *partials;      /* device; component-major partial rows */
  size_t partial_stride; /* doubles between components */
  int max_rows;          /* at most this many workgroups may leave a row */
  int required_rows;     /* > 0: exactly this many rows */
  void *stream;          /* hipStream_t of the context */
} mi_fused_args;
typedef int (*mi_apply_fused_fn)(void *user, const mi_vec *in, mi_vec *out, const mi_fused_args *args, int *rows);
MI_API int mi_op_create_callback_fused(mi_ctx *ctx, size_t n, mi_apply_fn fn, mi_apply_fused_fn fused, void *user,
                                       mi_op **out);
MI_API int mi_op_create_diag(mi_ctx *ctx, const mi_vec *d, mi_op **out);           /* Hp = d .* p */
MI_API int mi_op_create_csr(mi_ctx *ctx, const mi_csr *A, int p, mi_op **out);     /* Hp = A p    */
/* out = outer(inner(in)): e.g. TNLS's right-preconditioned LSQR operators A = dF o M, A' = M' o dF^* (reference
 * TNLS.h:60-63,432-447) as ONE device operator each, so that the inner solve stays in mi_lsqr.  Borrows both operands
 * (they must outlive the composition); owns one pooled intermediate vector. */
MI_API int mi_op_create_compose(mi_ctx *ctx, mi_op *outer, mi_op *inner, mi_op **out);
MI_API int mi_op_apply(mi_op *op, const mi_vec *in, mi_vec *out);
MI_API int mi_op_dims(const mi_op *op, size_t *n_in, size_t *n_out); /* either pointer may be null */
MI_API int mi_op_destroy(mi_op *op);

MI_API int mi_precon_create_callback(mi_ctx *ctx, size_t n, mi_apply_fn fn, void *user,
                                     mi_precon **out);
MI_API int mi_precon_create_diag(mi_ctx *ctx, const mi_vec *dinv, mi_precon **out); /* v = dinv .* r */
/* 3x3 block-Jacobi: blocks holds N row-major 3x3 INVERSE diagonal blocks (9N doubles) */
MI_API int mi_precon_create_block3(mi_ctx *ctx, const mi_vec *inv_blocks, mi_precon **out);
/* Constraint preconditioner of the PROJECTED solve (IterativeSolvers.h:83-85, applied at :229-253 and :381-405;
 * tests/IterativeSolvers_unit_test.cpp:316-496): P(r) = (v, lambda) with [M A'; A 0][v; lambda] = [r; 0] for a
 * DIAGONAL M (Minv = its inverse, n doubles) and a dense m x n constraint matrix A (row-major, m <= 512 <= n).
 * S = A M^-1 A' is formed, factored and inverted once on the device (sync); every application is two launches.
 * mi_precon_apply gives v; mi_precon_constraint_solve also lambda; mi_precon_constraint_At is A' (the `At` argument
 * of STPCG).  Handed to mi_stpcg with params.constraint_At != 0 the solve takes the reference's `At` branch
 * (r -= A' lambda after every preconditioner application, :251,403) inside the same pass.  A and Minv must outlive P. */
MI_API int mi_precon_create_constraint(mi_ctx *ctx, size_t n, size_t m, const mi_vec *A_rowmajor,
                                       const mi_vec *Minv_diag, mi_precon **out);
/* The same for SPARSE constraints and any number of them (r04): A (m x n) in CSR on the host (int32), M still diagonal.
 * A, A' and S = A M^-1 A' (formed once, on the host, as a sparse matrix) live on the device; an application is three
 * launches and no host round trip: b = A M^-1 r, then S lambda = b by a Jacobi-preconditioned CG iteration running
 * inside ONE workgroup (fixed-order reductions: deterministic) to a relative residual of inner_tol (0: 1e-14 -- the
 * projection must be accurate to rounding or the outer iterates drift out of the null space of A) or
 * inner_max_iterations (0: 10 m + 100), then v = M^-1 (r - A' lambda) and, with constraint_At, r -= A' lambda.
 * mi_precon_constraint_info reports what the inner iteration needed and left (sync).  Minv must outlive P.
 * Failure semantics (r06): a BREAKDOWN of the inner iteration (p'Sp <= 0 or not finite: dependent constraint rows, NaN /
 * Inf in the residual; status code 1) makes the mi_stpcg / mi_stpcg_collect that used the preconditioner return
 * MI_ERR_INTERNAL -- its result is not a projected step.  Stopping at inner_max_iterations short of inner_tol (status
 * code 2) is NOT an error: the caller who caps the iteration count gets the inexact projection it asked for, the solve
 * returns MI_OK with mi_stpcg_result::precon_status = 2, and mi_precon_constraint_info -- which always returns MI_OK on
 * a valid handle -- gives the code and the worst relative residual so far.  The status word is per solve (reset at the
 * start of each mi_stpcg). */
MI_API int mi_precon_create_constraint_csr(mi_ctx *ctx, size_t n, size_t m, const int32_t *rowptr, const int32_t *col,
                                           const double *val, const mi_vec *Minv, double inner_tol,
                                           size_t inner_max_iterations, mi_precon **out);
MI_API int mi_precon_constraint_info(mi_precon *P, size_t *last_inner_iterations, double *last_relative_residual,
                                     double *worst_relative_residual, int *status_code /* 0, 1 or 2; any pointer may
                                     be null */);
MI_API int mi_precon_constraint_solve(mi_precon *P, const mi_vec *r, mi_vec *v, mi_vec *lambda /*nullable*/);
MI_API int mi_precon_constraint_At(mi_precon *P, const mi_vec *lambda, mi_vec *out);
MI_API int mi_precon_apply(mi_precon *P, const mi_vec *r, mi_vec *v);
MI_API int mi_precon_destroy(mi_precon *P);

/* ---------------------------------------------------------------------------------------------
 * (5) fused Steihaug-Toint truncated preconditioned CG -- LinearAlgebra::STPCG
 *     (IterativeSolvers.h:166-426, unconstrained form: At == nullopt), metric = Euclidean/Frobenius
 *     dot of the coordinate arrays.  Device-resident scalar recurrences (:259-279,330-345,412-417);
 *     the host only polls a pinned status word and keeps `run_ahead` iterations enqueued.
 * ------------------------------------------------------------------------------------------- */
typedef struct mi_stpcg_params {
  double Delta;          /* :171 */
  size_t max_iterations; /* :172 (1000) */
  double kappa_fgr;      /* :172 (.1) */
  double theta;          /* :172 (.5) */
  double epsilon;        /* :179 (1e-8) */
  int run_ahead;         /* iterations the host may enqueue beyond the last one known complete (0 -> default 3) */
  int constraint_At;     /* nonzero: P is a constraint preconditioner (mi_precon_create_constraint) and the solve was given
                            `At` (IterativeSolvers.h:178): r -= A' lambda after every application of P (:251,403) */
  int defer_result;      /* nonzero: do NOT wait for the device at the exit.  s_out is valid in stream order (anything
                            enqueued afterwards sees it); `result` only receives hvp_calls, the other fields arrive
                            through mi_stpcg_collect.  Lets a caller put its next launch chain (e.g. the trust-region
                            trial step, Riemannian/TNT.h:493-512) behind the solve and read both back with ONE wait. */
} mi_stpcg_params;

enum {
  MI_STPCG_EXIT_RESIDUAL = 0, /* :290 */
  MI_STPCG_EXIT_MAXIT = 1,    /* :285 loop exhausted */
  MI_STPCG_EXIT_KERNEL = 2,   /* :305-337 */
  MI_STPCG_EXIT_BOUNDARY = 3, /* :347-361 */
  MI_STPCG_EXIT_USER = 4      /* :365-369, the observer of mi_stpcg_observed said stop */
};

typedef struct mi_stpcg_result {
  double update_step_M_norm; /* :334,359,424 */
  size_t num_iterations;     /* :285 (not incremented on boundary exits) */
  int exit_reason;
  size_t hvp_calls;          /* operator applications ENQUEUED (incl. speculative ones past the exit: it depends on when the
                                host saw the exit and may differ by a few between runs, by one in an observed solve) */
  double rv_final;           /* last <r,v> */
  int precon_status;         /* 0, or 2: a constraint preconditioner's inner iteration stopped at its iteration limit short
                                of its tolerance during this solve (an INEXACT projection; mi_precon_constraint_info has
                                the residual left).  A breakdown (code 1) makes mi_stpcg return MI_ERR_INTERNAL instead */
} mi_stpcg_result;

typedef struct mi_stpcg_trace { /* optional per-iteration scalars, host arrays of capacity cap */
  size_t cap, len;
  double *alpha, *beta, *kappa, *rv;
} mi_stpcg_trace;

MI_API void mi_stpcg_default_params(mi_stpcg_params *p);
/* sync at exit.  s_out must have g's length.  Returns MI_ERR_INVALID_ARGUMENT for the argument
 * ranges the reference rejects (:183-205). */
MI_API int mi_stpcg(mi_ctx *ctx, const mi_vec *g, mi_op *H, mi_precon *P /*nullable*/,
                    const mi_stpcg_params *params, mi_vec *s_out, mi_stpcg_result *result,
                    mi_stpcg_trace *trace /*nullable*/);
/* The same solve with the reference's STPCGUserFunction (IterativeSolvers.h:50-59) as a C callback: logging, custom
 * stopping rules, time limits inside the inner solve.  The observer is called once per pass after alpha_k is known and
 * the boundary tests have passed, before any update (:365-369) -- not in a pass that leaves by the kernel-of-H or the
 * boundary exit, as in the reference.  s, r, v, p are read-only views owned by the solve, valid for the duration of the
 * call: the step so far, the model gradient g + H s, the preconditioned residual (v == r, the same handle, when there is
 * no preconditioner, :231) and the direction; k is the number of completed updates.  A non-zero return stops the solve
 * like the reference's `break` (:369): s_out stays s_k, update_step_M_norm = sqrt(s_M_s) (:424), num_iterations = k,
 * exit_reason = MI_STPCG_EXIT_USER.
 *   Contract.  The observer runs on the calling thread with the stream drained up to this pass's operator.  On the same
 * context it may call the read-only vector functions on the views (mi_vec_dot, mi_vec_dot_batch, mi_vec_download,
 * mi_vec_copy FROM a view) and the plain applications mi_op_apply(H, view, own vector) / mi_precon_apply(P, view, own
 * vector) of the solve's operator and of an ordinary (diagonal, block, callback, Stiefel) preconditioner -- e.g. for the
 * model value <g,s> + <s,Hs>/2: the plain application of every built-in operator leaves the partial rows alone that
 * k_cg_update still has to reduce after the observer returns, and a user operator's plain callback (mi_apply_fn) is not
 * given them.  It must not write or destroy the views, must not apply a constraint preconditioner (its status word and
 * multipliers belong to the running solve), and must not call anything else that computes on that context: mi_stpcg /
 * mi_stpcg_observed are refused with MI_ERR_INVALID_ARGUMENT; mi_lsqr, the LOBPCG building blocks, the *_model / *_trial
 * chains and everything built on them (TNT, TNLS, GradientDescent) are NOT checked and share the reduction buffers and
 * the scalar file with the running solve.  A C++ exception must not leave it.
 *   What runs.  The kernels of mi_stpcg -- operator pass with fused dots, k_cg_update, k_cg_pupdate, direction-Gram
 * recurrence and its re-anchoring, every preconditioner kind incl. constraint_At -- and the same bits: with an observer
 * that never stops, s_out, the result and the trace equal mi_stpcg's.  What differs: no run-ahead (run_ahead is
 * ignored).  Between the operator and k_cg_update of every pass a one-workgroup kernel re-reduces the three curvature
 * sums, repeats the scalar step on a copy of the state and hands {alpha_k, decision} to the host through pinned words
 * and the polled flag: one small kernel and one polled wait per pass (mi_ctx_sync_count rises by one per pass; kernel
 * timing id MI_K_CG_SCALAR_A).  DEFER_S, EARLY_S, TWO_KERNEL_STEP and params->defer_result are off for an observed solve.
 *   Returns MI_DECLINED -- nothing done, nothing counted -- on a context that is one of several ranks or completes its
 * reductions through an exchange layer, with MI355OPT_FORCE_LOCKSTEP / FORCE_SLOT_PATH, and with MI355OPT_NO_FUSED_OBSERVER=1
 * (the A/B switch of the template layer): the caller keeps its generic loop. */
/* the small query behind that: MI_OK, or MI_DECLINED with *why (nullable) pointing at a literal that names the cause */
MI_API int mi_stpcg_observer_available(mi_ctx *ctx, const char **why);
typedef int (*mi_stpcg_observer)(void *user, size_t k, const mi_vec *s, const mi_vec *r, const mi_vec *v,
                                 const mi_vec *p, double alpha);
MI_API int mi_stpcg_observed(mi_ctx *ctx, const mi_vec *g, mi_op *H, mi_precon *P /*nullable*/,
                             const mi_stpcg_params *params, mi_stpcg_observer fn, void *user, mi_vec *s_out,
                             mi_stpcg_result *result, mi_stpcg_trace *trace /*nullable*/);
/* Result of the last mi_stpcg call made with defer_result on this context (update_step_M_norm :334,359,424,
 * num_iterations :285, exit reason, last <r,v>).  Waits only if the state copy enqueued at the solve's exit has not
 * completed yet -- after any later read-back on the same context it has.  (trace is not available in deferred mode.) */
MI_API int mi_stpcg_collect(mi_ctx *ctx, mi_stpcg_result *result);

/* ---------------------------------------------------------------------------------------------
 * (5b) fused LSQR  <->  LinearAlgebra::LSQR  IterativeSolvers.h:552-855 (Paige & Saunders, damped,
 *      with the trust-region radius of :779-793 and the stopping rules S1-S4 of :825-837; the user
 *      function S5 through mi_lsqr_observed).  Device-resident like mi_stpcg: no scalar reaches the
 *      host inside the loop of mi_lsqr.  A: n_x -> n_y, At: n_y -> n_x.
 * ------------------------------------------------------------------------------------------- */
typedef struct mi_lsqr_params {
  size_t max_iterations; /* :558 (1000) */
  double lambda;         /* :558 (0)    */
  double btol, Atol;     /* :558-559 (1e-6) */
  double Acond_limit;    /* :559 (1e8)  */
  double Delta;          /* :559 (sqrt(DBL_MAX)) */
  int run_ahead;         /* as in mi_stpcg_params */
} mi_lsqr_params;
enum {
  MI_LSQR_EXIT_MAXIT = 0,   /* loop exhausted (:696) */
  MI_LSQR_EXIT_S1 = 1,      /* :825 */
  MI_LSQR_EXIT_S2 = 2,      /* :829 */
  MI_LSQR_EXIT_S3 = 3,      /* :833 */
  MI_LSQR_EXIT_S4 = 4,      /* :837 */
  MI_LSQR_EXIT_TRIVIAL = 5, /* A'b = 0: x = 0 returned before the loop (:671-674) */
  MI_LSQR_EXIT_USER = 6     /* :845-851, the observer of mi_lsqr_observed said stop */
};
typedef struct mi_lsqr_result {
  double xnorm;          /* :769-770,793 */
  size_t num_iterations; /* :696 (not advanced by the pass that breaks) */
  int exit_reason;
  double rbar_norm, Arnorm, Anorm, Acond; /* :814,818,711,808 */
  size_t operator_applications;           /* enqueued, incl. speculative ones past the exit */
} mi_lsqr_result;
MI_API void mi_lsqr_default_params(mi_lsqr_params *p);
MI_API int mi_lsqr(mi_ctx *ctx, mi_op *A, mi_op *At, const mi_vec *b, const mi_lsqr_params *params,
                   mi_vec *x_out, mi_lsqr_result *result); /* sync at exit */
/* The same solve with the reference's LSQRUserFunction (IterativeSolvers.h:450-456) as a C callback.  The observer is
 * called at the end of every pass, all quantities updated, behind the stopping rules S1-S4 (:825-851): with x after this
 * pass's update, the loop index k of the pass (0, 1, ...) and |x|, |rbar|, |Abar' rbar|, the |Abar| and cond(Abar)
 * estimates.  Not in a pass that leaves through S1-S4, as in the reference; the pass that reaches max_iterations without
 * a stopping rule is observed (the reference's loop body completes before its `for` condition fails).  x is a read-only
 * view owned by the solve (x_out itself), valid for the duration of the call.  A non-zero return stops the solve like
 * the reference's `break` (:849-851): x_out keeps this pass's update, num_iterations = k (not advanced, also when the
 * pass was the last one allowed), exit_reason = MI_LSQR_EXIT_USER.
 *   Contract.  The observer runs on the calling thread with the stream drained up to this pass's k_lsqr_xw.  On the same
 * context it may call the read-only vector functions on the view (mi_vec_dot, mi_vec_dot_batch, mi_vec_download,
 * mi_vec_copy FROM the view) and the plain applications mi_op_apply(A or At, vector, own vector) -- e.g. for the true
 * residual b - A x.  It must not write or destroy the view and must not call anything else that computes on that
 * context: mi_lsqr / mi_lsqr_observed are refused with MI_ERR_INVALID_ARGUMENT; mi_stpcg, the LOBPCG building blocks, the
 * *_model / *_trial chains and everything built on them are NOT checked and share the reduction buffers with the running
 * solve.  A C++ exception must not leave it.
 *   What runs.  The kernels of mi_lsqr (k_lsqr_u, _unorm, _v, _vnorm, _xw, the fused-SpMV forms of the built-in CSR
 * operators) and the same bits: with an observer that never stops, x_out and the result equal mi_lsqr's.  What differs:
 * no run-ahead (run_ahead is ignored).  Behind k_lsqr_xw of every pass a one-wave kernel copies the state's
 * {mode, exit_reason, k, xnorm, rbar_norm, Arnorm, Anorm, Acond} into pinned host words and releases the polled flag: one
 * small kernel and one polled wait per pass (mi_ctx_sync_count rises by one per pass).  operator_applications is exact
 * for an observed solve: 1 + 2 * (passes enqueued), nothing speculative -- passes = num_iterations at a MAXIT exit,
 * num_iterations + 1 where S1-S4 or the observer ended the pass (mi_lsqr's count includes its run-ahead and depends on
 * timing).
 *   Returns MI_DECLINED -- nothing done, nothing counted -- on a context that is one of several ranks or completes its
 * reductions through an exchange layer, with MI355OPT_FORCE_LOCKSTEP, and with MI355OPT_NO_FUSED_LSQR_OBSERVER=1 (the A/B
 * switch of the template layer): the caller keeps its generic loop. */
/* the small query behind that: MI_OK, or MI_DECLINED with *why (nullable) pointing at a literal that names the cause */
MI_API int mi_lsqr_observer_available(mi_ctx *ctx, const char **why);
typedef int (*mi_lsqr_observer)(void *user, size_t k, const mi_vec *x, double xnorm, double rbar_norm, double Arnorm,
                                double Anorm, double Acond);
MI_API int mi_lsqr_observed(mi_ctx *ctx, mi_op *A, mi_op *At, const mi_vec *b, const mi_lsqr_params *params,
                            mi_lsqr_observer fn, void *user, mi_vec *x_out, mi_lsqr_result *result);


/* ---------------------------------------------------------------------------------------------
 * (6) Stiefel manifold St(n,p), 1 <= p <= 16, embedded metric -- the callables a client of
 *     TNT supplies (Objective, QuadraticModel, RiemannianMetric, Retraction; sphere analogue in
 *     the reference: tests/TNT_unit_test.cpp:73-117).  p <= 4: rows in registers, 1024-thread workgroups, the
 *     LDS-window form of the one-pass Hessian for p <= 3; p = 5 ... 8: the wide-row one-pass Hessian (256-thread
 *     workgroups, the p x p matrices in LDS) in STPCG's recurrence form, the two-pass operator with a preconditioner;
 *     p = 9 ... 16: the tall-row family (16 x 16 tiles on the fp64 matrix pipe, p a run-time argument): the two-pass
 *     operator with the curvature dots fused into its finish pass, on ONE context -- with a communicator, a
 *     row-sharded matrix or MI355OPT_FORCE_SLOT_PATH these widths are refused (MI_ERR_INVALID_ARGUMENT)
 * ------------------------------------------------------------------------------------------- */
MI_API int mi_stiefel_gram(mi_ctx *ctx, size_t n, int p, const mi_vec *X, const mi_vec *Z,
                           double *G_host /* p*p row-major, sync */);
MI_API int mi_stiefel_project(mi_ctx *ctx, size_t n, int p, const mi_vec *X, const mi_vec *Z,
                              mi_vec *out); /* Z - X sym(X'Z) */
MI_API int mi_stiefel_retract(mi_ctx *ctx, size_t n, int p, const mi_vec *X, const mi_vec *V,
                              mi_vec *Y);   /* polar: (X+V) ((X+V)'(X+V))^-1/2 */
/* f(X) = .5 tr(X' A X) */
MI_API int mi_stiefel_rq_create(mi_ctx *ctx, const mi_csr *A, size_t n, int p, mi_stiefel_rq **out);
MI_API int mi_stiefel_rq_destroy(mi_stiefel_rq *prob);
MI_API int mi_stiefel_rq_objective(mi_stiefel_rq *prob, const mi_vec *X, double *f); /* sync */
/* QuadraticModel: grad = AX - X sym(X'AX); caches S = sym(X'AX) on the device and binds the
 * Hessian operator  Hess[V] = P_X(A V - V S)  to X (X must outlive the operator's use). */
MI_API int mi_stiefel_rq_model(mi_stiefel_rq *prob, const mi_vec *X, mi_vec *grad, mi_op **hess);
/* One trial step at the point X the model is bound to -- the statements between the inner solve and the
 * accept/reject decision of Riemannian/TNT.h:493-512 (|h|, x_trial = retract(x, h), f(x_trial), <g,h>, <h, Hess h>)
 * plus, speculatively, the model at the trial point (:573-585: gradient and its norm) -- as one launch chain with ONE
 * read-back (sync).  out[5] = {f(X+), <h,h>, <g,h>, <h,Hess h>, |grad f(X+)|^2}.  A following
 * mi_stiefel_rq_model(prob, X_trial, ...) reuses A X+, S+ and the gradient instead of recomputing them.  Every number
 * has the bits the separate calls would produce. */
MI_API int mi_stiefel_rq_trial(mi_stiefel_rq *prob, const mi_vec *X, const mi_vec *h, const mi_vec *g,
                               mi_vec *X_trial, double out[5]);
/* One Armijo trial of a backtracking line search along -g (Riemannian/GradientDescent.h:266-286: h = -t g, x_trial =
 * retract(x, h), f(x_trial)) plus, speculatively, the gradient at the trial point and its squared norm (:325-327):
 * one launch chain, ONE read-back (sync).  out[2] = {f(X+), |grad f(X+)|^2}; h_out receives -t g.  A following
 * mi_stiefel_rq_model(prob, X_trial, ...) reuses what was computed. */
MI_API int mi_stiefel_rq_armijo_trial(mi_stiefel_rq *prob, const mi_vec *X, const mi_vec *g, double t, mi_vec *h_out,
                                      mi_vec *X_trial, double out[2]);
/* row-scaling (Jacobi) preconditioner projected to the tangent space: v = P_X(dinv_rows .* r) */
MI_API int mi_stiefel_rq_precon(mi_stiefel_rq *prob, const mi_vec *X, const mi_vec *dinv_rows,
                                mi_precon **out);

/* ---------------------------------------------------------------------------------------------
 * (7) SO(3)^N chordal rotation averaging  f(R) = .5 sum_e w_e |R_j - R_i Rt_e|_F^2
 * ------------------------------------------------------------------------------------------- */
MI_API int mi_so3n_create(mi_ctx *ctx, size_t N, size_t n_edges, const int32_t *ei,
                          const int32_t *ej, const double *Rt /*9 per edge*/, const double *w,
                          mi_so3n **out); /* sync (upload) */
MI_API int mi_so3n_destroy(mi_so3n *prob);
MI_API int mi_so3n_objective(mi_so3n *prob, const mi_vec *R, double *f); /* sync */
/* QuadraticModel: gradient in so(3)^N coordinates, Hessian operator as a symmetric 3x3-block
 * sparse matrix rebuilt at R, optional 3x3 block-Jacobi preconditioner from its diagonal blocks */
MI_API int mi_so3n_model(mi_so3n *prob, const mi_vec *R, mi_vec *grad, mi_op **hess,
                         mi_precon **block_jacobi /*nullable*/);
MI_API int mi_so3n_retract(mi_so3n *prob, const mi_vec *R, const mi_vec *xi, mi_vec *Y);
/* One trial step at the point R the model is bound to (Riemannian/TNT.h:493-512: |h|, R_trial = retract(R, h),
 * f(R_trial), <g,h>, <h, Hess h>) plus, speculatively, the model at the trial point (:573-585: gradient, Hessian blocks,
 * block-Jacobi blocks, |grad|^2 and -- with_precon -- |M^-1 grad|^2 with the preconditioner rebuilt there): one launch
 * chain, ONE read-back (sync).  out[6] = {f(R+), <h,h>, <g,h>, <h,Hess h>, |grad f(R+)|^2, |M+^-1 grad f(R+)|^2 or -1}.
 * A following mi_so3n_model(prob, R_trial, ...) swaps the speculative model in instead of rebuilding it.  Every number
 * has the bits the separate calls would produce. */
MI_API int mi_so3n_trial(mi_so3n *prob, const mi_vec *R, const mi_vec *h, const mi_vec *g, int with_precon,
                         mi_vec *R_trial, double out[6]);
/* VectorField (Riemannian/GradientDescent.h:216,325): grad f(R) in so(3)^N coordinates through the gradient-only form
 * of the assembly pass -- no Hessian blocks, no diagonal blocks, no model bound; no sync.  The bits of the gradient
 * mi_so3n_model writes.  If R is the point the last mi_so3n_armijo_trial evaluated the gradient found there is copied
 * and nothing is assembled; likewise for the point of the last mi_so3n_trial, whose speculative model stays in place
 * for a following mi_so3n_model(prob, R, ...). */
MI_API int mi_so3n_gradient(mi_so3n *prob, const mi_vec *R, mi_vec *grad);
/* One Armijo trial of a backtracking line search along -g (Riemannian/GradientDescent.h:266-286: h = -t g, R_trial =
 * retract(R, h), f(R_trial)) plus, speculatively, the gradient at the trial point and its squared norm (:323-327): one
 * launch chain, ONE read-back (sync).  out[2] = {f(R+), |grad f(R+)|^2}; h_out receives -t g.  Needs no bound model.
 * A following mi_so3n_gradient(prob, R_trial, ...) copies the gradient; a following mi_so3n_model(prob, R_trial, ...)
 * assembles the full model (only the gradient exists).  R_trial must not alias R, h_out must not alias g.  Every number
 * has the bits the separate calls (mi_vec_scale_to, mi_so3n_retract, mi_so3n_objective, mi_so3n_gradient, mi_vec_dot)
 * would produce. */
MI_API int mi_so3n_armijo_trial(mi_so3n *prob, const mi_vec *R, const mi_vec *g, double t, mi_vec *h_out,
                                mi_vec *R_trial, double out[2]);
/* The same problem as a nonlinear least-squares one, f(R) = 1/2 |F(R)|^2 (Riemannian/TNLS.h: Mapping, JacobianPairFunction):
 *   F(R)_e = sqrt(w_e) (R_j - R_i Rt_e), 9 doubles (row-major) per edge e = (i -> j) in the caller's edge order.
 * Needs w >= 0.  mi_so3n_residual is the Mapping F of TNLS.h:265 (F(x) at :399 and F(x_trial) at :553); sqnorm_or_null
 * receives |F(R)|^2 from the partial rows of the same pass (sync) -- null: no sync.  Reads R (or, at the point of the
 * last fused trial step, its quaternion records) and writes nothing that a Jacobian handed out earlier reads. */
MI_API int mi_so3n_residual(mi_so3n *prob, const mi_vec *R, mi_vec *F_out, double *sqnorm_or_null);
/* The Jacobian pair of TNLS.h:269,414-426 at R, as the two operators of LSQR's bidiagonalisation
 * (LinearAlgebra/IterativeSolvers.h:707 u = A v - alpha u, :712 v = A' u - beta v: both have apply_sub_scaled forms):
 *   (dF xi)_e = sqrt(w_e) (R_j hat(xi_j) - R_i hat(xi_i) Rt_e)                                      3N -> 9E
 *   (dF* Y)_i = sum over the incidences of node i, in their fixed slot order, of
 *               -sqrt(w_e) vee(R_i' Y_e Rt_e')  where i is the first node of e,  +sqrt(w_e) vee(R_i' Y_e)  where the second
 * with vee(M) = (M7 - M5, M2 - M6, M3 - M1).  No atomics: the same bits on every run.  Both handles are owned by the
 * problem (borrowed) and rebound by every call; they read a copy of the rotations taken by this call, so R may be
 * written, and the residual evaluated elsewhere, while they are in use.  dF has the 3-dimensional null space of the
 * global rotation; LSQR returns the minimum-norm step.  n_edges = 0 is MI_ERR_INVALID_ARGUMENT.  The first call uploads
 * the per-edge streams and the incidence -> edge map (sync); later calls do not synchronise. */
MI_API int mi_so3n_jacobian(mi_so3n *prob, const mi_vec *R, mi_op **dF, mi_op **dFt);
/* The right preconditioner pair (M, M') of TNLS.h:60-63 for this problem, M = M' = diag(1 / sqrt(2 degw_i)) (each entry
 * three times; 1 for a node of weighted degree 0): the diagonal blocks of dF* dF are exactly 2 degw_i I (|R hat(xi) S|^2 =
 * 2 |xi|^2), so this is the block-Jacobi scaling of the Gauss-Newton system.  Point-independent; owned by the problem. */
MI_API int mi_so3n_gn_scaling(mi_so3n *prob, mi_op **M);
/* Global-optimality certificate (as in SE-Sync).  With Y in R^{3N x 3}, Y_i = R_i', and Lap the 3N x 3N connection
 * Laplacian (diagonal blocks degw_i I, block (i, j) = -w_e Rt_e and (j, i) = -w_e Rt_e' for e = (i -> j)), f(R) = const +
 * 1/2 tr(Y' Lap Y), and the certificate matrix at R is
 *   S(R) = Lap - BlockDiag(C_i),  C_i = sym(Q_i),  Q_i = R_i' (L R)_i
 *   (S v)_i = (degw_i I - C_i) v_i - sum over the incidences of node i, in their fixed slot order, of w_e M' v_nbr
 * with M = Rt_e' where i is the first node of e and Rt_e where the second.  At every R: tr(Y' S Y) = 0, |S Y|_F =
 * |skew Q|_F (the stationarity defect, skew Q_i = (Q_i - Q_i') / 2), and f(R') >= f(R) + (3N / 2) min(lambda_min(S), 0)
 * for every R' in O(3)^N -- so S positive semidefinite at a critical point R certifies the global minimum.
 * mi_so3n_certificate forms the point-dependent part of S at R in one pass (the walk and the objective partials of
 * mi_so3n_objective) and returns info[3] = {f(R) with the bits of mi_so3n_objective, |skew Q|_F, sum_i tr C_i}: ONE
 * read-back (sync).  The handle is owned by the problem (borrowed) and rebound by the next call; it reads a COPY of what
 * depends on R (the blocks degw_i I - C_i, the panel Y), so later trial steps, model calls and writes to R leave it as it
 * is.  n_edges = 0 is allowed (S = 0).  Single-context only. */
typedef struct mi_so3n_cert mi_so3n_cert;
struct mi_panel_blocks;
MI_API int mi_so3n_certificate(mi_so3n *prob, const mi_vec *R, mi_so3n_cert **out, double info[3]);
/* Z = S X on column-major 3N x k panels (ld = 3N, 1 <= k <= 96), no sync, no atomics.  Each column is summed in one fixed
 * order -- the diagonal block, then the incidences in slot order -- and depends on the same column of X alone: column c of
 * Z has the same bits whatever k, pass or column-block split produced it.  Z must not overlap X.  The _blocks form takes
 * the input as 1 to 3 column blocks (mi_panel_blocks, section (8)): the same columns, the same bits. */
MI_API int mi_so3n_cert_apply(mi_so3n_cert *cert, int k, const mi_vec *X, mi_vec *Z);
MI_API int mi_so3n_cert_apply_blocks(mi_so3n_cert *cert, const struct mi_panel_blocks *X, mi_vec *Z);
/* The 3N x 3 column-major panel Y (Y(3i + r, c) = R_i[c][r]) at the certificate's point: S Y = 0 at a critical point, so
 * these are the three eigenvectors at (or near) 0 -- the start block of an eigensolver deflates them.  Borrowed. */
MI_API int mi_so3n_cert_null_panel(mi_so3n_cert *cert, mi_vec **Y);
/* Spectral initialisation: a start point from the three lowest eigenvectors of the connection Laplacian Lap (above), each
 * 3 x 3 block rounded to the nearest rotation.  Outside the method and NOT detected: a disconnected graph, weights <= 0.
 * mi_so3n_laplacian: Lap as a handle of the certificate's type -- mi_so3n_cert_apply and mi_so3n_cert_apply_blocks work on
 * it unchanged (the same kernel, the same bit contract); mi_so3n_cert_null_panel on it is MI_ERR_INVALID_ARGUMENT (it has no
 * Y).  Owned by the problem in a slot of its own: mi_so3n_certificate does not rebind it, nor the other way round.  Every
 * call refreshes the diagonal degw_i from the weights in force (after mi_so3n_reweight: the reweighted Laplacian), summed
 * per node in slot order, no atomics, no sync.  Single-context only. */
MI_API int mi_so3n_laplacian(mi_so3n *prob, mi_so3n_cert **out);
/* Z = D^-1 X on column-major 3N x k panels (ld = 3N, 1 <= k <= 96), D = degw_i on the three rows of node i: the Jacobi
 * preconditioner of Lap.  A node with degw_i = 0 copies.  The bits of X / degw; Z may be X; no sync.  Reads the diagonal of
 * the latest mi_so3n_laplacian call (formed here on first use). */
MI_API int mi_so3n_lap_jacobi(mi_so3n *prob, int k, const mi_vec *X, mi_vec *Z);
/* R_i = the rotation nearest in the Frobenius norm to M_i = V[3i .. 3i+2, :]' of the column-major 3N x 3 panel V (the
 * layout of mi_so3n_cert_null_panel), U diag(1, 1, det(U V')) V' for M_i = U Sigma V': a block with det < 0 has its smallest
 * singular direction flipped.  Global sign first: when sum_i sign(det V_i) < 0 (an integer, counted on the device) -V is
 * rounded instead -- a basis in the reflected gauge spans the same space; a tie does not flip.  A block with a non-finite
 * entry, the zero block, or a block whose projection is not finite (rank one) becomes the identity and is counted as
 * degenerate.  R: the 9N point (row-major blocks), not overlapping V.
 * info (nullable) = {blocks with det V_i < 0 as given, flipped (0 / 1), degenerate blocks, min over the other blocks of
 * (sigma_2 + d sigma_3) / sigma_1, d the sign of the determinant of the block that was rounded (NaN when every block is
 * degenerate)}: one read-back (sync); info == NULL: no sync. */
MI_API int mi_so3n_round(mi_so3n *prob, const mi_vec *V, mi_vec *R, double info[4]);
/* The same projection block by block on a 9N point M (a user-supplied or drifted point with an orthogonality defect), no
 * global sign; R may be M.  info (nullable) = {max over the non-degenerate blocks of |M_i' M_i - I|_F, degenerate blocks,
 * blocks with det < 0}: one read-back (sync); info == NULL: no sync. */
MI_API int mi_so3n_project(mi_so3n *prob, const mi_vec *M, mi_vec *R, double info[3]);
/* Robust loss by iteratively reweighted least squares: the edge weights become w_e = w0_e phi(r_e) on the device, with
 * w0_e the creation-time weight, r_e = |R_j - R_i Rt_e|_F the UNWEIGHTED chordal residual at R, s = r_e^2 / c^2 and
 *   MI_ROBUST_L2             phi = 1                          rho = r^2 / 2
 *   MI_ROBUST_HUBER          phi = 1 (r <= c), c / r (r > c)  rho = r^2 / 2 (r <= c), c r - c^2 / 2 (r > c)
 *   MI_ROBUST_CAUCHY         phi = 1 / (1 + s)                rho = (c^2 / 2) log1p(s)
 *   MI_ROBUST_GEMAN_MCCLURE  phi = 1 / (1 + s)^2              rho = (r^2 / 2) / (1 + s)
 * (rho' = r phi: a minimiser of sum w0 rho(r) is a fixed point of solve / reweight rounds).  Graduated non-convexity with
 * the Geman-McClure surrogate, w = (mu c^2 / (r^2 + mu c^2))^2, is MI_ROBUST_GEMAN_MCCLURE called with c sqrt(mu): it needs
 * no kind of its own.  Two passes, no atomics (the same bits on every run): one thread per edge, then one lane per node
 * rewriting the per-incidence weights (and, where they exist, sqrt(w_e) of the least-squares view and the diagonal of
 * mi_so3n_gn_scaling).  Every entry point of this section then computes what a problem created with the weights
 * mi_so3n_weights returns computes.
 * w_e <- w0_e * phi(|R_j - R_i Rt_e|_F ; kind, c).  info (nullable) = {sum w0 rho(r), sum w r^2/2, #edges with phi < 1/2}:
 * one read-back (sync); info == NULL: no sync.  R may be NULL for MI_ROBUST_L2 (restores the creation-time weights; info is
 * then formed with r = 0).  The first call uploads the creation-time weights, the per-edge streams and the incidence -> edge
 * map (sync).
 * A reweighting drops the bound model, the speculative model of the last mi_so3n_trial and the gradient of the last
 * mi_so3n_armijo_trial: a following mi_so3n_model on any vector assembles afresh, and mi_so3n_trial needs a new
 * mi_so3n_model first.  The handle of mi_so3n_certificate and the pair of mi_so3n_jacobian were formed with the old weights
 * and must be requested again; the handle of mi_so3n_gn_scaling stays valid and sees the new scaling.
 * MI_ERR_INVALID_ARGUMENT (weights untouched): an unknown kind; c not finite or <= 0 for a kind other than MI_ROBUST_L2; R
 * of the wrong length or context, or NULL for such a kind; a context with a communicator (single-context only).
 * n_edges = 0 is allowed (info = 0). */
enum { MI_ROBUST_L2 = 0, MI_ROBUST_HUBER = 1, MI_ROBUST_CAUCHY = 2, MI_ROBUST_GEMAN_MCCLURE = 3 };
MI_API int mi_so3n_reweight(mi_so3n *prob, const mi_vec *R, int kind, double c, double info[3]);
MI_API int mi_so3n_weights(mi_so3n *prob, double *w_host /* E */);   /* sync: the current w_e */

/* ---------------------------------------------------------------------------------------------
 * (7b) pose-graph translations: with the rotations R fixed (the 9N point of mi_so3n), the positions of a pose graph with
 *     edges e = (i -> j), relative translations tt_e (3 per edge) and weights tau_e >= 0 solve the linear least-squares problem
 *         min_t  f_tau(R, t) = 1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2    <=>    L_a t = b(R),   t_anchor = 0
 *     (second stage of chordal initialisation; what SE-Sync does after its rotation solve).  L_a is the tau-weighted graph
 *     Laplacian with the anchor's row and column -- and the row of every node of weighted degree 0 -- replaced by the unit
 *     row, acting on the N x 3 row-major field t.  Refused (MI_ERR_INVALID_ARGUMENT, with a message): an anchor or an end
 *     point outside [0, N), a self-loop, a non-finite tt, a tau that is negative or not finite, a context with a
 *     communicator (single-context only).  Outside the method and NOT detected: several components that carry edges (CG
 *     returns a solution of the consistent singular system).
 * ------------------------------------------------------------------------------------------- */
typedef struct mi_pgo_trans mi_pgo_trans;
typedef struct mi_pgo_trans_info {
  size_t iterations;        /* of the PCG solve */
  int exit_reason;          /* MI_STPCG_EXIT_*: RESIDUAL is convergence; MAXIT, KERNEL and BOUNDARY are reported, not errors */
  double objective;         /* f_tau(R, t_out) */
  double relative_residual; /* |L_a t_out - b| / |b| from ONE plain application after the solve, not the recurrence (|b| = 0:
                               |L_a t_out|) */
  double max_residual;      /* max_e | t_j - t_i - R_i tt_e | at t_out */
} mi_pgo_trans_info;
/* sync (upload).  Owns its mi_csr (L_a), the mi_op of mi_op_create_csr(ctx, L_a, 3) and the mi_precon of
 * mi_precon_create_diag (1 / diagonal, each value three times). */
MI_API int mi_pgo_trans_create(mi_ctx *ctx, size_t N, size_t n_edges, const int32_t *ei, const int32_t *ej,
                               const double *tt /* 3 per edge */, const double *tau, long long anchor, mi_pgo_trans **out);
MI_API int mi_pgo_trans_destroy(mi_pgo_trans *T);
/* b (3N) = the right-hand side at R (9N); b_anchor = 0 and b = 0 on nodes of weighted degree 0.  One lane per node, the
 * incidences summed in slot order, no atomics: the same bits on every run.  No sync. */
MI_API int mi_pgo_trans_rhs(mi_pgo_trans *T, const mi_vec *R, mi_vec *b);
/* Borrowed handles (mi_op_destroy / mi_precon_destroy on them are no-ops; they live as long as T), for a caller's own
 * mi_stpcg: L_a on 3N-vectors with the curvature dots fused, and its Jacobi preconditioner (fused into the CG update).
 * Either pointer may be null. */
MI_API int mi_pgo_trans_operator(mi_pgo_trans *T, mi_op **L, mi_precon **jacobi);
/* r_e = t_j - t_i - R_i tt_e in the caller's edge order into r_out (3E; may be NULL: nothing written, the same out bits);
 * out = {f_tau(R, t), max_e |r_e|}, both reduced in a fixed order.  One read-back (sync). */
MI_API int mi_pgo_trans_residual(mi_pgo_trans *T, const mi_vec *R, const mi_vec *t, mi_vec *r_out, double out[2]);
/* t_out (3N) = the positions: rhs, then mi_stpcg used as plain PCG from t = 0 (g = -b, a radius that never binds, theta = 0,
 * kappa_fgr = tol: the stop sqrt(<r,v>) <= tol sqrt(<r0,v0>), 0 <= tol < 1), then the residual pass.  t_out[anchor] = 0 and
 * t_out = 0 on nodes of weighted degree 0, exactly.  Sync. */
MI_API int mi_pgo_trans_solve(mi_pgo_trans *T, const mi_vec *R, double tol, size_t max_iterations, mi_vec *t_out,
                              mi_pgo_trans_info *info);

/* ---------------------------------------------------------------------------------------------
 * (7c) pose-graph refinement on SE(3)^N: rotations and positions together,
 *         f(R, t) = 1/2 sum_e kappa_e | R_j - R_i Rt_e |_F^2  +  1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2,   e = (i -> j).
 *     Point: 12N doubles [R | t] -- the first 9N in the layout of mi_so3n, the last 3N in the layout of mi_pgo_trans, so a
 *     mi_vec_view of either half goes to mi_so3n_* / mi_pgo_trans_* and back without a copy.  Tangent: 6N doubles, node-major
 *     [xi_i (3), delta_i (3)]: the point moves as R_i exp(hat xi_i), t_i + delta_i; the metric is the coordinate dot.  No
 *     gauge is fixed (the Hessian is semidefinite along the global motions).  kappa is taken as mi_so3n_create takes w.
 *     Refused (MI_ERR_INVALID_ARGUMENT, with a message): an end point outside [0, N), a self-loop, a non-finite tt, a tau
 *     that is negative or not finite, a context with a communicator (single-context only).
 * ------------------------------------------------------------------------------------------- */
typedef struct mi_pgo mi_pgo;
MI_API int mi_pgo_create(mi_ctx *ctx, size_t N, size_t n_edges, const int32_t *ei, const int32_t *ej,
                         const double *Rt /* 9 per edge */, const double *tt /* 3 per edge */, const double *kappa,
                         const double *tau, mi_pgo **out); /* sync (upload) */
MI_API int mi_pgo_destroy(mi_pgo *prob);
MI_API int mi_pgo_objective(mi_pgo *prob, const mi_vec *x, double *f); /* sync */
/* grad f(x) (6N) through the gradient-only form of the assembly pass: the bits of the gradient mi_pgo_model writes; no sync */
MI_API int mi_pgo_gradient(mi_pgo *prob, const mi_vec *x, mi_vec *grad);
/* QuadraticModel: the gradient, the Hessian operator assembled at x (one fused pass per product, the curvature dots inside
 * for mi_stpcg) and the 3x3 block-Jacobi preconditioner of its 2N diagonal blocks (a block without an inverse is replaced
 * by the identity).  Both handles are borrowed and live as long as prob; either pointer may be null.  No sync. */
MI_API int mi_pgo_model(mi_pgo *prob, const mi_vec *x, mi_vec *grad, mi_op **hess, mi_precon **block_jacobi);
/* y = [R_i exp(hat xi_i) | t_i + delta_i]; y must not alias x.  No sync. */
MI_API int mi_pgo_retract(mi_pgo *prob, const mi_vec *x, const mi_vec *eta, mi_vec *y);
/* One trial step at the point x the model is bound to (Riemannian/TNT.h:493-512, 573-585): one launch chain, ONE read-back
 * (sync).  out[6] = {f(x+), <h,h>, <g,h>, <h,Hess h>, |grad f(x+)|^2, |M+^-1 grad f(x+)|^2 with the inverse blocks rebuilt
 * at x+ (with_precon) or -1}.  Every number has the bits the separate calls (mi_op_apply + mi_vec_dot, mi_pgo_retract,
 * mi_pgo_objective, mi_pgo_gradient, mi_precon_apply) would produce.  The model stays bound to x: a following
 * mi_pgo_model(prob, x_trial, ...) assembles afresh. */
MI_API int mi_pgo_trial(mi_pgo *prob, const mi_vec *x, const mi_vec *h, const mi_vec *g, int with_precon, mi_vec *x_trial,
                        double out[6]);

/* ---------------------------------------------------------------------------------------------
 * (8) LOBPCG building blocks (LinearAlgebra/LOBPCG.h:131-337).  Panels are column-major m x k
 *     (ld = m), matching the reference's Eigen dense layout.
 * ------------------------------------------------------------------------------------------- */
/* G (ka x kb, column-major, host, sync) = S' * AS  -- LOBPCG.h:223,271-272 ; fp64 MFMA */
MI_API int mi_lobpcg_gram(mi_ctx *ctx, size_t m, int ka, int kb, const mi_vec *S, const mi_vec *AS,
                          double *G_host);
/* The same for T = [T1 (m x k1) | T2 (m x (k - k1))] held in two panels, G = S' T (k x k): the reference's S' A(S)
 * (LOBPCG.h:267,271) with A(S) = [A(X) | A([W P])] where A(X) is the panel of the previous iteration (:281) -- the same
 * columns, hence the same bits, one operator application fewer.  sync */
MI_API int mi_lobpcg_gram_split(mi_ctx *ctx, size_t m, int k, const mi_vec *S, int k1, const mi_vec *T1,
                                const mi_vec *T2, double *G_host);
/* Both Grams of a Rayleigh-Ritz step (LOBPCG.h:271-272: S'AS and S'BS) with ONE synchronisation: enqueued back to
 * back, read back together.  Each right-hand panel is one panel of k columns (T?2 == NULL, k1? ignored) or two
 * pieces [T?1 (k1? columns) | T?2].  Same kernels, same bits as the separate calls.  sync */
MI_API int mi_lobpcg_gram_pair(mi_ctx *ctx, size_t m, int k, const mi_vec *S, int k1a, const mi_vec *Ta1,
                               const mi_vec *Ta2, int k1b, const mi_vec *Tb1, const mi_vec *Tb2, double *Ga_host,
                               double *Gb_host);
/* The same for the case every LOBPCG iteration without a B operator is in: G_a = S' [Ta1 | Ta2] with T = A S for a
 * SYMMETRIC operator A (the reference's SymmetricLinearOperator, LOBPCG.h:131-134) and G_b = S' S, LOBPCG.h:271-272.
 * Both are symmetric; only the upper block triangle of each is formed (16 x 16 tiles; the lower block triangle is its
 * mirror image, which is also all the reference's eigensolver reads), from ONE pass over S and T.  Ta2 may be null. */
MI_API int mi_lobpcg_gram_pair_sym(mi_ctx *ctx, size_t m, int k, const mi_vec *S, int k1a, const mi_vec *Ta1,
                                   const mi_vec *Ta2, double *Ga_host, double *Gb_host);
/* A panel held as 1 to 3 column blocks that need not be adjacent: block i = the first cols[i] columns of block[i] (a
 * panel, or a mi_vec_view of some columns of one).  LOBPCG's search basis S = [X, W(:, nc:), P(:, nc:)]
 * (LOBPCG.h:254-264) is handed over like this -- as its three blocks lie -- instead of being copied together every
 * iteration once pairs are locked (nc > 0).  The *_blocks entry points below compute what their namesakes compute on
 * the concatenation of the blocks; shapes their one-pass kernels do not take are copied together internally. */
typedef struct mi_panel_blocks {
  int nblocks;
  const mi_vec *block[3];
  int cols[3];
} mi_panel_blocks;
MI_API int mi_lobpcg_gram_pair_sym_blocks(mi_ctx *ctx, size_t m, const mi_panel_blocks *S, int k1a, const mi_vec *Ta1,
                                          const mi_vec *Ta2, double *Ga_host, double *Gb_host);
/* mi_lobpcg_gram_pair_sym_blocks with T = A(S) held as column blocks as well (a plain-callable operator applied to the
 * blocks of S one by one). */
MI_API int mi_lobpcg_gram_pair_sym_tblocks(mi_ctx *ctx, size_t m, const mi_panel_blocks *S, const mi_panel_blocks *T,
                                           double *Ga_host, double *Gb_host);
/* The generalized problem (a B operator, LOBPCG.h:131-140,268,272; tests/LOBPCG_unit_test.cpp:178-225): the upper block
 * triangles of S' A(S) and S' B(S) -- both symmetric, SymmetricLinearOperator -- with S, A(S) and B(S) each held as column
 * blocks of the same total width ([X | W(:, nc:) | P(:, nc:)], [AX | A(W..) | A(P..)], [BX | B(W..) | B(P..)]): nothing is
 * copied together (r05).  One launch per Gram on the matrix pipe, one reduction, one read-back. */
MI_API int mi_lobpcg_gram_pair_gen_blocks(mi_ctx *ctx, size_t m, const mi_panel_blocks *S, const mi_panel_blocks *AS,
                                          const mi_panel_blocks *BS, double *Ga_host, double *Gb_host);
MI_API int mi_lobpcg_update2_blocks(mi_ctx *ctx, size_t m, const mi_panel_blocks *S, int kc, const double *C_host,
                                    int ldc, mi_vec *Y, int k1, mi_vec *Y2);
MI_API int mi_csr_spmm_colmajor_blocks(const mi_csr *A, const mi_panel_blocks *X, mi_vec *Y);
/* Y (m x kc) = S (m x ks) * C (ks x kc column-major host) -- LOBPCG.h:226-227,278,288 */
MI_API int mi_lobpcg_update(mi_ctx *ctx, size_t m, int ks, int kc, const mi_vec *S,
                            const double *C_host, int ldc, mi_vec *Y);
/* The same with two destinations: output columns [0, k1) -> Y (m x k1), [k1, kc) -> Y2 (m x (kc - k1)).  Lets the
 * LOBPCG loop write X and P (LOBPCG.h:278,288) straight into the first and third block of the NEXT search basis
 * instead of copying them there (:254-259). */
MI_API int mi_lobpcg_update2(mi_ctx *ctx, size_t m, int ks, int kc, const mi_vec *S, const double *C_host, int ldc,
                             mi_vec *Y, int k1, mi_vec *Y2);
/* R = AX - BX diag(theta); rnorm[j] = |R_j|, xnorm[j] = |X_j| (host, sync) -- LOBPCG.h:230,285,293,302 */
MI_API int mi_lobpcg_residual(mi_ctx *ctx, size_t m, int nx, const mi_vec *AX, const mi_vec *BX,
                              const mi_vec *X, const double *theta_host, mi_vec *R, double *rnorm,
                              double *xnorm);
/* Rayleigh-Ritz on the host (ns <= 96): LOBPCG.h:53-62.  Theta ascending, C'AC = Theta, C'BC = I */
MI_API int mi_rayleigh_ritz(int n, const double *A, const double *B, double *Theta, double *C);
/* The k LOWEST Ritz pairs only: Theta[k] ascending, C n x k column-major with C'AC = diag(Theta), C'BC = I.  An LOBPCG
 * iteration reads nx of the ns <= 3 nx pairs (LOBPCG.h:278,288,293-318); same reduction, same QL recurrence (the Ritz
 * values have the bits of mi_rayleigh_ritz), the vectors from the recorded rotations applied to k columns instead of n
 * (they agree with the full solver's columns to rounding).  Host, like mi_rayleigh_ritz. */
MI_API int mi_rayleigh_ritz_lowest(int n, int k, const double *A, const double *B, double *Theta, double *C);
/* Y (n x k column-major) = A X : the sparse operator of LOBPCG clients (called at LOBPCG.h:213,218,267,281) */
MI_API int mi_csr_spmm_colmajor(const mi_csr *A, int k, const mi_vec *X, mi_vec *Y);
/* AX (n x nx) = A X (LOBPCG.h:281) together with R = AX - X diag(theta) (:285, B absent so BX = X) and the column norms
 * of R and X (:293,302; host, sync): when the matrix takes the LDS-window form the residual is finished in the
 * product's own pass (the row's X values are in the ring), otherwise this is mi_csr_spmm_colmajor followed by
 * mi_lobpcg_residual.  R has the same bits either way. */
MI_API int mi_csr_spmm_colmajor_residual(const mi_csr *A, int nx, const mi_vec *X, const double *theta_host,
                                         mi_vec *AX, mi_vec *R, double *rnorm, double *xnorm);
/* Y[r,c] = d[r] X[r,c] : diagonal operator / Jacobi preconditioner on a column-major panel
 * (the operators of tests/LOBPCG_unit_test.cpp:56-74) */
MI_API int mi_panel_rowscale(mi_ctx *ctx, size_t m, int k, const mi_vec *d, const mi_vec *X, mi_vec *Y);

/* ---------------------------------------------------------------------------------------------
 * (9) multi-GPU: one process per GPU, tangent vectors row-sharded, inner products completed by an
 *     in-stream RCCL all-reduce of the scalar slots.  uid = ncclUniqueId bytes
 *     obtained on rank 0 with mi_comm_unique_id and broadcast by the launcher.
 * ------------------------------------------------------------------------------------------- */
#define MI_COMM_UID_BYTES 128
MI_API int mi_comm_unique_id(unsigned char uid[MI_COMM_UID_BYTES]);
MI_API int mi_comm_init(mi_ctx *ctx, int world_size, int rank,
                        const unsigned char uid[MI_COMM_UID_BYTES]); /* sync */
MI_API int mi_comm_finalize(mi_ctx *ctx);
MI_API int mi_comm_info(mi_ctx *ctx, int *world_size, int *rank);
/* ranks of the RCCL communicator as RCCL itself reports them (ncclCommCount); 0: no RCCL communicator attached */
MI_API int mi_comm_rccl_count(mi_ctx *ctx, int *nranks);
/* Peer-memory layer for the tiny, latency-bound exchanges of the STPCG path (scalar all-reduces, halo
 * rows): every rank exports one fine-grained device arena (hipIpcGetMemHandle), the launcher gathers
 * the handles, every rank maps all of them (hipIpcOpenMemHandle: plain xGMI peer stores), runs the
 * collective self-test, and the layer is enabled only if EVERY rank passed (the launcher reduces the
 * verdicts); otherwise RCCL keeps doing those exchanges.  Also works without RCCL (mi_comm_init not
 * called): that is how several ranks on ONE GPU are tested (RCCL refuses duplicate devices). */
#define MI_COMM_IPC_HANDLE_BYTES 64
MI_API int mi_comm_ipc_export(mi_ctx *ctx, unsigned char handle[MI_COMM_IPC_HANDLE_BYTES]);
MI_API int mi_comm_ipc_attach(mi_ctx *ctx, int world_size, int rank,
                              const unsigned char *handles /* world_size x MI_COMM_IPC_HANDLE_BYTES */);
/* Collective, sync.  Known-value all-reduces and all-gathers through the exchange kernel, then (world_size > 1) the
 * FOLDED forms between the real peers: the scalar exchange inside a streaming kernel's prologue and all three forms of
 * the halo push (early fold, late fold, separate kernel) over 24 rounds with a consumer that checks every halo double.
 * The caller must combine the ranks' verdicts (a collective: no rank may go on before every rank is through) and pass
 * the result to mi_comm_ipc_enable on every rank. */
MI_API int mi_comm_ipc_selftest(mi_ctx *ctx, int *ok);
MI_API int mi_comm_ipc_enable(mi_ctx *ctx, int on);
MI_API int mi_comm_ipc_error(mi_ctx *ctx, int *err);        /* nonzero: a bounded wait timed out */
/* exchanges folded into their producer / consumer kernels (default on; env MI355OPT_NO_FOLD=1: off) switched at run
 * time -- every rank must make the same call between the same two solves.  Results are bit-identical either way. */
MI_API int mi_comm_ipc_fold(mi_ctx *ctx, int on);
/* Kernels the peer-memory layer launched on its own so far: out[0] scalar-exchange kernels, out[1] halo-push kernels,
 * out[2] halo pushes that rode in the kernel producing the vector instead (no launch), out[3] those of out[2] in the
 * EARLY form (the producer walks its vector starting at the neighbours' rows and signals after its first step).
 * With folding on (the default) a sharded fused STPCG iteration adds nothing to out[0] and out[1]: it is the three
 * kernels of the single-GPU step. */
MI_API int mi_comm_kernel_launches(mi_ctx *ctx, unsigned long long out[4]);
/* Verification hooks (used by tests/test_gpu_comm.py on a ONE-GPU box): pretend to be `rank` of
 * `world_size` WITHOUT a communicator, and fill a sharded matrix's halo rows by hand, so that the halo
 * addressing of the sparse kernels can be checked against the global product.  Not part of the drop-in
 * surface; with a communicator the halo is filled by the in-stream ncclSend/ncclRecv exchange. */
/* which form of the sparse kernels a matrix got: out = {window half-width in 64-row chunks (0: none), widest slice, far
 * stride D when every entry outside the window is at row +- D (the kernels then compute those columns, halo columns
 * of a row shard included) else 0, halo rows} */
MI_API int mi_debug_csr_window_info(const mi_csr *A, size_t out[4]);
/* read-only: what the value-indexed formats of a matrix hold: out = {packed copy (0 / 1), entries of the value table,
 * index of 0.0 (the one the window words use where there is a window form: the table's size when 0.0 had to be
 * appended; else its place in the table, SIZE_MAX when it has none), 16-bit window words (0 / 1), the stride in rows
 * shared by >= 80 % of the entries outside the window or 0} */
MI_API int mi_debug_csr_format_info(const mi_csr *A, size_t out[5]);
/* read-only: the forms an SO(3)^N problem took -- {measurements stored as unit quaternions, neighbours gathered as
 * quaternions, slices, incidences, padded incidence slots, workgroups of the model assembly}; needs no GPU work */
MI_API int mi_debug_so3n_info(const mi_so3n *q, size_t out[6]);
/* Host only (no device needed): the layout csrc/pgo_pack.h builds for a problem of mi_pgo_create, from one run of the
 * packer.  counts = {N, E, slices, incidences, padded slots}; arrays 0 ... 7 = slice_ptr (long long), perm, nbr (int), the slot
 * words (uint32_t), rinc, tinc, kinc, tauinc (double): n[a] = the number of elements of array a; up to cap[a] of them are copied
 * to out[a].  out may be NULL (sizes only). */
MI_API int mi_debug_pgo_pack(size_t N, size_t n_edges, const int32_t *ei, const int32_t *ej, const double *Rt,
                             const double *tt, const double *kappa, const double *tau, size_t counts[5], void *const out[8],
                             const size_t cap[8], size_t n[8]);
/* The three curvature sums of ONE fused pass of the joint Hessian (the form mi_stpcg drives): h = H eta with the workgroup
 * partial rows reduced in row order; out = {<eta,h>, <h,h>, <eta,eta>}.  Needs an assembled model.  Sync. */
MI_API int mi_debug_pgo_hvp_dots(mi_pgo *prob, const mi_vec *eta, mi_vec *h, double out[3]);
/* What the last mi_pgo_model wrote (sync).  which = 0: kappa B per slot, 1: the coupling blocks per slot (padded * 9 each),
 * 2: the node blocks in slice order (slices * 19 * 64), 3: the 2N inverse blocks (18N), 4: the inverse blocks the last
 * mi_pgo_trial with with_precon left at its trial point.  info (nullable) = {slices, incidences, padded slots, workgroups
 * of the assembly}. */
MI_API int mi_debug_pgo_blocks(mi_pgo *prob, int which, double *out, size_t cap, size_t *count, size_t info[4]);
/* Test hook: one application of the operator's fused LSQR form (IterativeSolvers.h:707,712: inout = Op(in) - scale inout
 * with |inout|^2 from the same pass) driven as mi_lsqr drives it; nothing happens when mode != 0.  MI_DECLINED when the
 * operator has no such form.  sync. */
MI_API int mi_debug_op_apply_sub_scaled(mi_op *op, const mi_vec *in, double scale, int mode, mi_vec *inout,
                                        double *sqnorm);
/* host-only: the run plan of the LDS-window kernels (first tile of every run + the end) for `ntiles` tiles of 256 rows,
 * a workgroup budget, a CU count and the matrix's far stride in rows (0: none); needs no GPU */
MI_API int mi_debug_window_runs(int ntiles, int max_wgs, int num_cu, size_t far_stride, int *bounds_out, int cap,
                                int *nb_out);
/* host-only, read-only: the launch plan of the Stiefel one-pass Hessian for rows of p doubles and a gram_count (-1: the
 * recurrence form, -2: that of the two-kernel step, >= 0: Gram rows of the direction kernel); needs no GPU.
 *   traits   = {packed copy, window words, 16-bit window words, window chunks, widest slice, pure far stride D,
 *               common far stride, halo buffer, row-sharded} of the matrix
 *   switches = {NO_WINDOW, NO_FAR_COMPUTED, WORDS16, WIDE_QUAD, WIDE_WINDOW, NO_WIN_BOUNDS, uniform grid, slot mode,
 *               the two-kernel step's residual is set} of the context
 *   out      = {form (0 k_st_hess_fused plain, 1 its window form, 2 k_st_hess_widewin, 3 k_st_hess_wide,
 *               4 k_st_hess_wideq), FROM_SLOTS, HALO, RECUR, PK, HW, FAR, TWOK, block size, dynamic LDS bytes, run table
 *               wanted, halo exchange first, Gram reduction first, the gram_count = -2 form exists}
 * A combination the library treats as an internal error is an error here too (MI_ERR_INVALID_ARGUMENT). */
MI_API int mi_debug_stiefel_hess_form(int p, int gram_count, const size_t traits[9], const int switches[9], int out[14]);
/* host-only, read-only: the same `out` for a matrix on a context as both stand -- what the library itself reads of them
 * (a context that has opted into TWO_KERNEL_STEP counts as WORDS16 = 0), so FAR = 2 says that this context's Hessian
 * pass streams the 16-bit words */
MI_API int mi_debug_stiefel_hess_form_of(const mi_ctx *ctx, const mi_csr *A, int p, int gram_count, int out[14]);
/* host-only, read-only: the launch plans of the LOBPCG building blocks (csrc/lobpcg_plan.h) for plain numbers; no GPU.
 * Flags are 0 / 1.
 *   kind 0, mi_lobpcg_gram:  in  = {m, ka, kb, S and T are one panel, T = [T1 | T2], every panel 16-byte aligned,
 *                                   every panel 32-byte aligned, compute units}
 *                            out = {ok (0: a split T on a shape the direct kernel does not take), direct (k_gram_direct,
 *                                   else k_gram), SAME, ALIGNED, k_gram_tail runs, T of k_gram_direct, TPW of k_gram,
 *                                   waves per SIMD, waves, partial Grams, rows in whole pipeline steps, LDS bytes}
 *   kind 1, the symmetric pair (k_gram_pair_sym): in = {m, k, both Grams in one launch (0: the generalized problem),
 *                                   NO_GRAM_HALF, compute units};  out = {T, HALF, PAIR, waves per SIMD, waves, rows in
 *                                   whole 16-row steps}
 *   kind 2, the eligibility rule of those kernels: in = {m, k, every column block 32-byte aligned, least row count};
 *                                   out = {eligible, least row count of k_gram_direct, of k_gram_pair_sym} */
MI_API int mi_debug_lobpcg_gram_plan(int kind, const size_t *in, size_t *out);
/* host-only: the plan of Y = S C for a basis of nblocks column blocks (cols[i] columns each) and kc output columns, and
 * the packed coefficients Ct of the column-major C (ks x kc, leading dimension ldc) as the kernels read them.
 *   all_mfma: the matrix-pipe kernel runs;  steps: nsteps x {block, first column within it, basis column behind each of
 *   the four coefficient rows or -1}, room for 18;  chunks: nchunks x {first output column, width, offset in Ct}, room
 *   for 4;  Ct: ct_len doubles, room for ct_cap */
MI_API int mi_debug_lobpcg_update_plan(size_t m, int kc, int nblocks, const int *cols, int no_update_mfma,
                                       const double *C_host, int ldc, int *all_mfma, int *nsteps, int *steps,
                                       int *nchunks, int *chunks, double *Ct, size_t ct_cap, size_t *ct_len);
/* host-only: the grid of the plane-sweep panel product for a far stride of D rows, n rows, k columns and SWEEP_ZSEGS
 * (0: chosen here): out = {the form takes this D (else the window form runs), tiles per plane, planes, passes, z-segments,
 * planes per segment, workgroups per pass} */
MI_API int mi_debug_lobpcg_sweep_plan(size_t D, size_t n, int k, int num_cu, int sweep_zsegs, int out[7]);
/* host-only: Config::words16 of a context created with MI355OPT_WORDS16 = text (NULL: unset); needs no GPU */
MI_API int mi_debug_words16_option(const char *text, int *on);
MI_API int mi_debug_set_rank(mi_ctx *ctx, int world_size, int rank);
MI_API int mi_debug_csr_set_halo(mi_csr *A, int p, const double *halo_rows_host); /* (need_lo+need_hi) x p */
/* Measurement hook: average microseconds of `reps` back-to-back applications of the operator in the fused form
 * mi_stpcg uses (the user HVP of IterativeSolvers.h:294 together with the dots of :300,305-306), timed with
 * events on the context stream.  sync.  Not part of the drop-in surface (tools/time_op.py). */
MI_API int mi_debug_time_fused_apply(mi_op *op, const mi_vec *in, mi_vec *out, int reps, double *us_per_call);
/* halo description for a row-sharded sparse operator: rows [row_begin,row_end) of a global n x n
 * matrix are local; columns outside are fetched from the owning neighbour before each SpMM */
/* host-only planning step of mi_csr_create_sharded (no GPU needed; also used by the CPU gloo tests):
 * halo extents + local column indices ([0,n) local, then halo from rank-1, then halo from rank+1) */
MI_API int mi_csr_shard_plan(size_t n_global, int world_size, int rank, const size_t *row_starts,
                             size_t nnz_local, const int64_t *col_global, int32_t *col_local, size_t *need_lo,
                             size_t *need_hi);
MI_API int mi_csr_create_sharded(mi_ctx *ctx, size_t n_global, size_t row_begin, size_t row_end,
                                 size_t nnz_local, const int32_t *rowptr, const int64_t *col_global,
                                 const double *val, const size_t *row_starts /*world_size+1*/,
                                 mi_csr **out);

#ifdef __cplusplus
}
#endif
#endif /* MI355OPT_H */
