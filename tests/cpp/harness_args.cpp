// harness_args.cpp -- the template layer called the way the reference's Riemannian clients call it: with an extra-argument
// pack (`Args &...`, Base/Concepts.h:20-38 -- a cache, a counter) behind x0.  Every driver is ONE template over the pack,
// instantiated with the empty pack and with a non-empty one, so that pytest can hold the two runs against each other:
// the tagged device callables ignore the pack, hence the same kernels on the same data and the same bits
// (tests/test_gpu_args_fusion.py).  The counting drivers also run on the plain host vector of oracle/template_driver.inc,
// where the template layer is the reference's statement sequence.  TEST INFRASTRUCTURE ONLY.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/LinearAlgebra/IterativeSolvers.h"
#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/MI355/Stiefel.h"
#include "Optimization/Riemannian/GradientDescent.h"
#include "Optimization/Riemannian/TNLS.h"
#include "Optimization/Riemannian/TNT.h"

#define DRV(name) hab_##name
#include "template_driver.inc"  // HostVec (and its drivers under the hab_ prefix, unused here)

using namespace Optimization;
using MI355::Context;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *ha_last_error() { return g_msg.c_str(); }

#define HA_GUARD_END                         \
  }                                          \
  catch (const std::invalid_argument &e) {   \
    g_msg = e.what();                        \
    return -1;                               \
  }                                          \
  catch (const std::exception &e) {          \
    g_msg = e.what();                        \
    return -2;                               \
  }                                          \
  return 0;

namespace {

struct ArgsOut {  // plain data, mirrored by ctypes in the test
  mi_fusion_counters fusion;  // of the run's own context, over the optimizer call
  size_t syncs;               // mi_ctx_sync_count over the optimizer call
  size_t accepted;            // accepted steps seen by the TNTUserFunction
  size_t user_calls;          // calls of the user function
  double seconds;             // wall time of the (last) optimizer call
};

void fill_params(RM::TNTParams<double> &tp, const orc_tnt_params *p) {
  tp.max_iterations = p->max_iterations;
  tp.max_computation_time = p->max_computation_time;
  tp.gradient_tolerance = p->gradient_tolerance;
  tp.relative_decrease_tolerance = p->relative_decrease_tolerance;
  tp.stepsize_tolerance = p->stepsize_tolerance;
  tp.Delta0 = p->Delta0;
  tp.eta1 = p->eta1;
  tp.eta2 = p->eta2;
  tp.alpha1 = p->alpha1;
  tp.alpha2 = p->alpha2;
  tp.max_TPCG_iterations = p->max_TPCG_iterations;
  tp.kappa_fgr = p->kappa_fgr;
  tp.theta = p->theta;
  tp.preconditioned_gradient_tolerance = p->preconditioned_gradient_tolerance;
  tp.Delta_tolerance = p->Delta_tolerance;
}

template <typename Vec>
void export_result(const RM::TNTResult<Vec, double> &r, const std::vector<double> &x, orc_tnt_result *res) {
  std::memcpy(res->x, x.data(), x.size() * sizeof(double));
  res->f = r.f;
  res->gradfx_norm = r.gradfx_norm;
  res->preconditioned_gradfx_norm = r.preconditioned_grad_f_x_norm;
  res->status = static_cast<int>(r.status);
  res->outer_iterations = r.inner_iterations.size();
  res->n_trace = r.objective_values.size();
  for (size_t i = 0; i < res->n_trace; ++i) {
    res->objective_values[i] = r.objective_values[i];
    res->gradient_norms[i] = r.gradient_norms[i];
    res->preconditioned_gradient_norms[i] = r.preconditioned_gradient_norms[i];
    res->trust_region_radius[i] = r.trust_region_radius[i];
  }
  for (size_t i = 0; i < res->outer_iterations; ++i) {
    res->inner_iterations[i] = r.inner_iterations[i];
    res->update_step_norms[i] = r.update_step_norms[i];
    res->update_step_M_norms[i] = r.update_step_M_norms[i];
    res->gain_ratios[i] = r.gain_ratios[i];
  }
}

// counters and synchronisations of `ctx` over one call
template <typename F>
auto counted(const Context &ctx, ArgsOut *out, F &&run) {
  mi_fusion_counters f0, f1;
  size_t c0 = 0, c1 = 0;
  ctx.synchronize();
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f0));
  MI355::check(mi_ctx_sync_count(ctx.get(), &c0));
  const auto t0 = std::chrono::steady_clock::now();
  auto r = run();
  out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  MI355::check(mi_ctx_sync_count(ctx.get(), &c1));
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f1));
  out->fusion.fused_stpcg_solves = f1.fused_stpcg_solves - f0.fused_stpcg_solves;
  out->fusion.generic_stpcg_solves = f1.generic_stpcg_solves - f0.generic_stpcg_solves;
  out->fusion.fused_lsqr_solves = f1.fused_lsqr_solves - f0.fused_lsqr_solves;
  out->fusion.generic_lsqr_solves = f1.generic_lsqr_solves - f0.generic_lsqr_solves;
  out->fusion.fused_trial_steps = f1.fused_trial_steps - f0.fused_trial_steps;
  out->fusion.generic_trial_steps = f1.generic_trial_steps - f0.generic_trial_steps;
  out->fusion.generic_inner_products = f1.generic_inner_products - f0.generic_inner_products;
  out->syncs = c1 - c0;
  return r;
}

// TNT on a problem object through its pack-templated accessors; the caller's pack behind x0 (reference TNT.h:242-252).
// wrap_hessian: the Hessian the model returns is wrapped in a lambda of the client's (the tag is lost).
template <typename Prob, typename... Args>
RM::TNTResult<DeviceVector, double> tnt_on(Prob &prob, const Context &ctx, const DeviceVector &x0,
                                           const RM::TNTParams<double> &tp, bool with_precon, bool wrap_hessian,
                                           int repeats, ArgsOut *out, Args &...args) {
  using Op = RM::LinearOperator<DeviceVector, DeviceVector, Args...>;
  std::optional<RM::TNTUserFunction<DeviceVector, DeviceVector, double, Args...>> uf =
      RM::TNTUserFunction<DeviceVector, DeviceVector, double, Args...>(
          [out](size_t, double, const DeviceVector &, double, const DeviceVector &, const Op &, double, size_t,
                const DeviceVector &, double, double, bool acc, Args &...) {
            out->accepted += acc;
            out->user_calls++;
            return false;
          });
  Objective<DeviceVector, double, Args...> f = prob.template objective<Args...>();
  RM::QuadraticModel<DeviceVector, DeviceVector, Args...> QM = prob.template quadratic_model<Args...>();
  RM::RiemannianMetric<DeviceVector, DeviceVector, double, Args...> metric = prob.template metric<Args...>();
  RM::Retraction<DeviceVector, DeviceVector, Args...> retract = prob.template retraction<Args...>();
  if (wrap_hessian) {
    auto QMt = QM;
    QM = [QMt](const DeviceVector &X, DeviceVector &g, Op &Hs, Args &...a) {
      Op tagged;
      QMt(X, g, tagged, a...);
      Hs = [tagged](const DeviceVector &Y, const DeviceVector &V, Args &...b) { return tagged(Y, V, b...); };
    };
  }
  std::optional<Op> pc;
  if constexpr (std::is_same<Prob, MI355::RotationAveraging>::value) {
    if (with_precon) pc = prob.template preconditioner<Args...>();
  }
  RM::TNTResult<DeviceVector, double> r;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); ++rep) {
    out->accepted = out->user_calls = 0;
    r = counted(ctx, out, [&] {
      return RM::TNT<DeviceVector, DeviceVector, double, Args...>(f, QM, metric, retract, x0, args..., pc, tp, uf);
    });
  }
  return r;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// TNT on St(n,p), f(X) = 1/2 tr(X'AX).  pack = 0: Args = {};  pack = 1: Args = {int, DeviceVector} (a tag and a cache
// vector of the client's, as in the reference's tests/TNT_unit_test.cpp:139).  wrap_hessian: see tnt_on.
// repeats > 1: the call is repeated in one context and the last run reported (benchmarks).
// ------------------------------------------------------------------------------------------------
extern "C" int ha_tnt_stiefel(size_t n, int p, const int32_t *rowptr, const int32_t *col, const double *val,
                              const double *X0, const orc_tnt_params *params, int pack, int wrap_hessian, int repeats,
                              orc_tnt_result *res, ArgsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    MI355::StiefelRayleighQuotient prob(ctx, n, p, rowptr, col, val);
    DeviceVector x0(ctx, X0, n * (size_t)p);
    RM::TNTParams<double> tp;
    fill_params(tp, params);
    RM::TNTResult<DeviceVector, double> r;
    if (pack == 0) {
      r = tnt_on<MI355::StiefelRayleighQuotient>(prob, ctx, x0, tp, false, wrap_hessian != 0, repeats, out);
    } else {
      int tag = 7;
      DeviceVector cache(ctx, std::vector<double>(5, 1.0));
      r = tnt_on<MI355::StiefelRayleighQuotient, int, DeviceVector>(prob, ctx, x0, tp, false, wrap_hessian != 0, repeats,
                                                                    out, tag, cache);
    }
    export_result(r, r.x.to_host(), res);
    res->accepted = out->accepted;
  HA_GUARD_END
}

// TNT on SO(3)^N rotation averaging with the problem's own block-Jacobi preconditioner.  pack = 1: Args = {DeviceVector}
extern "C" int ha_tnt_so3n(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w,
                           const double *R0, const orc_tnt_params *params, int pack, orc_tnt_result *res,
                           ArgsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    MI355::RotationAveraging prob(ctx, N, E, ei, ej, Rt, w);
    DeviceVector x0(ctx, R0, 9 * N);
    RM::TNTParams<double> tp;
    fill_params(tp, params);
    RM::TNTResult<DeviceVector, double> r;
    if (pack == 0) {
      r = tnt_on<MI355::RotationAveraging>(prob, ctx, x0, tp, true, false, 1, out);
    } else {
      DeviceVector cache(ctx, std::vector<double>(3, 0.5));
      r = tnt_on<MI355::RotationAveraging, DeviceVector>(prob, ctx, x0, tp, true, false, 1, out, cache);
    }
    export_result(r, r.x.to_host(), res);
    res->accepted = out->accepted;
  HA_GUARD_END
}

// ------------------------------------------------------------------------------------------------
// GradientDescent on the Stiefel Rayleigh quotient.  pack = 1: Args = {DeviceVector}
// ------------------------------------------------------------------------------------------------
namespace {
template <typename... Args>
RM::GradientDescentResult<DeviceVector, double> gd_on(MI355::StiefelRayleighQuotient &prob, const Context &ctx,
                                                      const DeviceVector &x0,
                                                      const RM::GradientDescentParams<double> &gp, ArgsOut *out,
                                                      Args &...args) {
  Objective<DeviceVector, double, Args...> f = prob.objective<Args...>();
  RM::VectorField<DeviceVector, DeviceVector, Args...> grad = prob.gradient<Args...>();
  RM::RiemannianMetric<DeviceVector, DeviceVector, double, Args...> metric = prob.metric<Args...>();
  RM::Retraction<DeviceVector, DeviceVector, Args...> retract = prob.retraction<Args...>();
  return counted(ctx, out, [&] {
    return RM::GradientDescent<DeviceVector, DeviceVector, double, Args...>(f, grad, metric, retract, x0, args..., gp);
  });
}
}  // namespace

extern "C" int ha_gd_stiefel(size_t n, int p, const int32_t *rowptr, const int32_t *col, const double *val,
                             const double *X0, size_t max_iterations, double gradient_tolerance, double alpha,
                             double beta, double sigma, size_t max_ls_iterations, int pack, double *x_out, double *f_out,
                             double *gradnorm_out, int *status_out, size_t *iterations_out, size_t cap,
                             double *objective_values, size_t *linesearch_iterations, ArgsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    MI355::StiefelRayleighQuotient prob(ctx, n, p, rowptr, col, val);
    DeviceVector x0(ctx, X0, n * (size_t)p);
    RM::GradientDescentParams<double> gp;
    gp.max_iterations = max_iterations;
    gp.gradient_tolerance = gradient_tolerance;
    gp.relative_decrease_tolerance = 0;
    gp.stepsize_tolerance = 0;
    gp.alpha = alpha;
    gp.beta = beta;
    gp.sigma = sigma;
    gp.max_ls_iterations = max_ls_iterations;
    RM::GradientDescentResult<DeviceVector, double> r;
    if (pack == 0) {
      r = gd_on(prob, ctx, x0, gp, out);
    } else {
      DeviceVector cache(ctx, std::vector<double>(4, 2.0));
      r = gd_on<DeviceVector>(prob, ctx, x0, gp, out, cache);
    }
    const std::vector<double> x = r.x.to_host();
    std::memcpy(x_out, x.data(), x.size() * sizeof(double));
    *f_out = r.f;
    *gradnorm_out = r.gradfx_norm;
    *status_out = static_cast<int>(r.status);
    *iterations_out = r.linesearch_iterations.size();
    for (size_t i = 0; i < r.objective_values.size() && i < cap; ++i) objective_values[i] = r.objective_values[i];
    for (size_t i = 0; i < r.linesearch_iterations.size() && i < cap; ++i)
      linesearch_iterations[i] = r.linesearch_iterations[i];
  HA_GUARD_END
}

// ------------------------------------------------------------------------------------------------
// LSQR with A and A' as two CSR operators, tagged callables.  pack = 1: Args = {int, DeviceVector}.
// (TNLS itself cannot be instantiated with a non-empty pack, here as in the reference: its J is declared without the
// pack, TNLS.h:269, and called with it, :422.)
// ------------------------------------------------------------------------------------------------
namespace {
template <typename... Args>
DeviceVector lsqr_on(const Context &ctx, mi_op *opA, mi_op *opAt, const DeviceVector &b, size_t max_iterations,
                     double lambda, double btol, double Atol, double Acond_limit, double Delta, double &xnorm,
                     size_t &iters, ArgsOut *out, Args &...args) {
  LA::LinearOperator<DeviceVector, DeviceVector, Args...> A = MI355::DeviceOperator{opA};
  LA::LinearOperator<DeviceVector, DeviceVector, Args...> At = MI355::DeviceOperator{opAt};
  LA::InnerProduct<DeviceVector, double, Args...> ip = MI355::FrobeniusInnerProduct{};
  return counted(ctx, out, [&] {
    return LA::LSQR<DeviceVector, DeviceVector, double, Args...>(A, At, b, ip, ip, args..., xnorm, iters, max_iterations,
                                                                 lambda, btol, Atol, Acond_limit, Delta);
  });
}
}  // namespace

extern "C" int ha_lsqr_csr(size_t n, const int32_t *rp, const int32_t *cl, const double *vl, const int32_t *rpt,
                           const int32_t *clt, const double *vlt, const double *b, size_t max_iterations, double lambda,
                           double btol, double Atol, double Acond_limit, double Delta, int pack, double *x_out,
                           double *xnorm_out, size_t *iterations_out, ArgsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    mi_csr *A = nullptr, *At = nullptr;
    MI355::check(mi_csr_create(ctx.get(), n, (size_t)rp[n], rp, cl, vl, &A));
    MI355::check(mi_csr_create(ctx.get(), n, (size_t)rpt[n], rpt, clt, vlt, &At));
    mi_op *opA = nullptr, *opAt = nullptr;
    MI355::check(mi_op_create_csr(ctx.get(), A, 1, &opA));
    MI355::check(mi_op_create_csr(ctx.get(), At, 1, &opAt));
    {
      DeviceVector bv(ctx, b, n);
      double xnorm = 0;
      size_t iters = 0;
      DeviceVector x;
      if (pack == 0) {
        x = lsqr_on(ctx, opA, opAt, bv, max_iterations, lambda, btol, Atol, Acond_limit, Delta, xnorm, iters, out);
      } else {
        int tag = 3;
        DeviceVector cache(ctx, std::vector<double>(2, 1.0));
        x = lsqr_on<int, DeviceVector>(ctx, opA, opAt, bv, max_iterations, lambda, btol, Atol, Acond_limit, Delta, xnorm,
                                       iters, out, tag, cache);
      }
      const std::vector<double> xh = x.to_host();
      std::memcpy(x_out, xh.data(), n * sizeof(double));
      *xnorm_out = xnorm;
      *iterations_out = iters;
    }
    mi_op_destroy(opA);
    mi_op_destroy(opAt);
    mi_csr_destroy(A);
    mi_csr_destroy(At);
  HA_GUARD_END
}

// ------------------------------------------------------------------------------------------------
// A pack that user code writes: Args = {size_t} -- a counter of the client's, handed by reference through the whole call
// chain and incremented by the user function.  One templated driver per solver, on HostVec (plain callables: the
// reference's statement sequence) and on DeviceVector (tagged callables: the fused paths).
// ------------------------------------------------------------------------------------------------
namespace {

struct CountOut {
  size_t counter;     // the caller's own object after the call
  size_t iterations;  // STPCG: num_iterations; TNT: outer iterations
  double M_norm;      // STPCG: |s|_M;  TNT: f at the returned point
  ArgsOut dev;        // device only
};

// STPCG<Vec, Mult, double, size_t> with a user function that increments the pack's counter and stops at stop_at
template <typename Vec>
Vec counting_stpcg(const Vec &g, const LA::SymmetricLinearOperator<Vec, size_t> &H,
                   const LA::InnerProduct<Vec, double, size_t> &ip,
                   const std::optional<LA::STPCGPreconditioner<Vec, Mult, size_t>> &P, double Delta, size_t max_iterations,
                   double kappa, double theta, size_t stop_at, CountOut *out) {
  size_t counter = 0;
  const std::optional<LA::LinearOperator<Mult, Vec, size_t>> At;
  std::optional<LA::STPCGUserFunction<Vec, Mult, double, size_t>> uf = LA::STPCGUserFunction<Vec, Mult, double, size_t>(
      [stop_at](size_t k, const Vec &, const LA::SymmetricLinearOperator<Vec, size_t> &,
                const std::optional<LA::STPCGPreconditioner<Vec, Mult, size_t>> &,
                const std::optional<LA::LinearOperator<Mult, Vec, size_t>> &, const Vec &, const Vec &, const Vec &,
                const Vec &, double, size_t &calls) {
        ++calls;
        return k == stop_at;
      });
  double mn = 0;
  size_t it = 0;
  Vec s = LA::STPCG<Vec, Mult, double, size_t>(g, H, ip, counter, mn, it, Delta, max_iterations, kappa, theta, P, At, uf);
  out->counter = counter;
  out->iterations = it;
  out->M_norm = mn;
  return s;
}

// TNT<Vec, Vec, double, Args...> on f(x) = <g,x> + <x, D x>/2 (flat metric, R_x(v) = x + v); with Args = {size_t} the
// TNTUserFunction increments the pack's counter
inline void bump() {}
inline void bump(size_t &calls) { ++calls; }
template <typename Vec, typename... Args>
RM::TNTResult<Vec, double> counting_tnt(const Objective<Vec, double, Args...> &f,
                                        const RM::QuadraticModel<Vec, Vec, Args...> &QM,
                                        const RM::RiemannianMetric<Vec, Vec, double, Args...> &metric, const Vec &x0,
                                        size_t max_iterations, Args &...args) {
  const RM::Retraction<Vec, Vec, Args...> retract = [](const Vec &x, const Vec &v, Args &...) { return x + v; };
  RM::TNTParams<double> tp;
  tp.max_iterations = max_iterations;
  tp.gradient_tolerance = 1e-6;
  tp.relative_decrease_tolerance = 0;
  tp.stepsize_tolerance = 0;
  tp.preconditioned_gradient_tolerance = 0;
  tp.Delta_tolerance = 0;
  tp.max_TPCG_iterations = 20;
  std::optional<RM::TNTUserFunction<Vec, Vec, double, Args...>> uf = RM::TNTUserFunction<Vec, Vec, double, Args...>(
      [](size_t, double, const Vec &, double, const Vec &, const RM::LinearOperator<Vec, Vec, Args...> &, double, size_t,
         const Vec &, double, double, bool, Args &...a) {
        bump(a...);
        return false;
      });
  return RM::TNT<Vec, Vec, double, Args...>(f, QM, metric, retract, x0, args...,
                                            std::optional<RM::LinearOperator<Vec, Vec, Args...>>(), tp, uf);
}

HostVec diag_times(size_t n, const double *D, const HostVec &v);

// the host side of it, plain callables in the pack's signature
template <typename... Args>
RM::TNTResult<HostVec, double> host_quadratic_tnt(size_t n, const double *g, const double *D, size_t max_iterations,
                                                  Args &...args) {
  const HostVec gh(g, n);
  Objective<HostVec, double, Args...> f = [&](const HostVec &x, Args &...) {
    return gh.dot(x) + .5 * x.dot(diag_times(n, D, x));
  };
  RM::QuadraticModel<HostVec, HostVec, Args...> QM =
      [&](const HostVec &x, HostVec &grad, RM::LinearOperator<HostVec, HostVec, Args...> &Hs, Args &...) {
        grad = gh + diag_times(n, D, x);
        Hs = [D, n](const HostVec &, const HostVec &v, Args &...) { return diag_times(n, D, v); };
      };
  RM::RiemannianMetric<HostVec, HostVec, double, Args...> metric =
      [](const HostVec &, const HostVec &a, const HostVec &b, Args &...) { return a.dot(b); };
  return counting_tnt<HostVec, Args...>(f, QM, metric, 0 * gh, max_iterations, args...);
}

HostVec diag_times(size_t n, const double *D, const HostVec &v) {
  HostVec o(n);
  for (size_t i = 0; i < n; ++i) o.d[i] = D[i] * v.d[i];
  return o;
}

}  // namespace

// solver = 0: STPCG (diagonal Hessian D, optional diagonal preconditioner Minv, stop at stop_at);
// solver = 1: TNT on the quadratic of the same g, D from x0 = 0 (Minv, Delta, kappa, theta, stop_at unused)
// pack = 0 (host vector, solver 1 only): the same call with the empty pack, no counter
extern "C" int ha_counting(int device, int solver, int pack, size_t n, const double *g, const double *D, const double *Minv,
                           double Delta, size_t max_iterations, double kappa, double theta, size_t stop_at,
                           double *s_out, CountOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    if (pack == 0 && (device || solver != 1)) throw std::invalid_argument("pack = 0 is the host TNT's only");
    if (!device) {
      const HostVec gh(g, n);
      if (solver == 0) {
        LA::SymmetricLinearOperator<HostVec, size_t> H = [&](const HostVec &v, size_t &) { return diag_times(n, D, v); };
        LA::InnerProduct<HostVec, double, size_t> ip = [](const HostVec &a, const HostVec &b, size_t &) {
          return a.dot(b);
        };
        std::optional<LA::STPCGPreconditioner<HostVec, Mult, size_t>> P;
        if (Minv)
          P = LA::STPCGPreconditioner<HostVec, Mult, size_t>(
              [&](const HostVec &v, size_t &) { return std::make_pair(diag_times(n, Minv, v), Mult()); });
        HostVec s = counting_stpcg<HostVec>(gh, H, ip, P, Delta, max_iterations, kappa, theta, stop_at, out);
        std::memcpy(s_out, s.d.data(), n * sizeof(double));
      } else {
        // (the empty pack: for the bit-for-bit comparison of the two host runs)
        size_t counter = 0;
        RM::TNTResult<HostVec, double> r = pack == 0 ? host_quadratic_tnt<>(n, g, D, max_iterations)
                                                        : host_quadratic_tnt<size_t>(n, g, D, max_iterations, counter);
        out->counter = counter;
        out->iterations = r.inner_iterations.size();
        out->M_norm = r.f;
        std::memcpy(s_out, r.x.d.data(), n * sizeof(double));
      }
      return 0;
    }
    Context ctx(0);
    DeviceVector gd(ctx, g, n), Dd(ctx, D, n);
    mi_op *op = nullptr;
    MI355::check(mi_op_create_diag(ctx.get(), Dd.handle(), &op));
    mi_precon *pc = nullptr;
    std::optional<DeviceVector> Mi;
    if (Minv && solver == 0) {
      Mi = DeviceVector(ctx, Minv, n);
      MI355::check(mi_precon_create_diag(ctx.get(), Mi->handle(), &pc));
    }
    if (solver == 0) {
      LA::SymmetricLinearOperator<DeviceVector, size_t> H = MI355::DeviceOperator{op};
      LA::InnerProduct<DeviceVector, double, size_t> ip = MI355::FrobeniusInnerProduct{};
      std::optional<LA::STPCGPreconditioner<DeviceVector, Mult, size_t>> P;
      if (pc) P = LA::STPCGPreconditioner<DeviceVector, Mult, size_t>(MI355::DeviceSTPCGPreconditioner<Mult>{pc});
      DeviceVector s = counted(ctx, &out->dev, [&] {
        return counting_stpcg<DeviceVector>(gd, H, ip, P, Delta, max_iterations, kappa, theta, stop_at, out);
      });
      const std::vector<double> sh = s.to_host();
      std::memcpy(s_out, sh.data(), n * sizeof(double));
    } else {
      // the client's own objective (a plain callable with the pack) on top of a tagged Hessian and the tagged metric: the
      // inner solves are fused, the trial step keeps the statement sequence
      Objective<DeviceVector, double, size_t> f = [&](const DeviceVector &x, size_t &) {
        return gd.dot(x) + .5 * x.dot(MI355::apply_device_operator(op, x));
      };
      RM::QuadraticModel<DeviceVector, DeviceVector, size_t> QM =
          [&](const DeviceVector &x, DeviceVector &grad, RM::LinearOperator<DeviceVector, DeviceVector, size_t> &Hs,
              size_t &) {
            grad = gd + MI355::apply_device_operator(op, x);
            Hs = MI355::DeviceHessian{op, nullptr};
          };
      RM::RiemannianMetric<DeviceVector, DeviceVector, double, size_t> metric = MI355::FrobeniusMetric{};
      size_t counter = 0;
      RM::TNTResult<DeviceVector, double> r = counted(ctx, &out->dev, [&] {
        return counting_tnt<DeviceVector, size_t>(f, QM, metric, 0 * gd, max_iterations, counter);
      });
      out->counter = counter;
      out->iterations = r.inner_iterations.size();
      out->M_norm = r.f;
      const std::vector<double> xh = r.x.to_host();
      std::memcpy(s_out, xh.data(), n * sizeof(double));
    }
    mi_op_destroy(op);
    if (pc) mi_precon_destroy(pc);
  HA_GUARD_END
}
