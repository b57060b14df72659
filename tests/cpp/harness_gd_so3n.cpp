// harness_gd_so3n.cpp -- Riemannian::GradientDescent<DeviceVector, DeviceVector, double, Args...> on MI355::RotationAveraging
// (chordal rotation averaging on SO(3)^N) through the problem object's accessors, the way a client of the drop-in
// headers writes it.  One templated driver, four modes:
//   0  objective(), gradient(), metric(), retraction(): the fused Armijo trial (mi_so3n_armijo_trial, one read-back per trial)
//   1  the same with plain_retraction(): the reference's statement sequence, still on prob.gradient()
//   2  mode 0 with Args = {DeviceVector} (a cache of the client's) through objective<DeviceVector>() etc.
//   3  mode 0 with the objective wrapped in a lambda (f + 1): the tag is lost, the statement sequence must run
// tests/test_gpu_so3n_gradient_descent.py holds the runs against each other and against tests/golden/gd_so3n.json.
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/GradientDescent.h"
#include "Optimization/Util/Stopwatch.h"

using namespace Optimization;
namespace RM = Optimization::Riemannian;
using MI355::Context;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *hg_last_error() { return g_msg.c_str(); }

namespace {

struct GdOut {  // plain data, mirrored by ctypes in tests/harness_gd_so3n_py.py
  mi_fusion_counters fusion;  // of the run's own context, over the optimizer call
  size_t syncs;               // mi_ctx_sync_count over the optimizer call
  double seconds;
};

template <typename... Args>
RM::GradientDescentResult<DeviceVector, double> gd_on(MI355::RotationAveraging &prob, const Context &ctx,
                                                      const DeviceVector &x0, const RM::GradientDescentParams<double> &gp,
                                                      bool plain_retraction, bool wrap_objective, GdOut *out,
                                                      Args &...args) {
  Objective<DeviceVector, double, Args...> f = prob.objective<Args...>();
  RM::VectorField<DeviceVector, DeviceVector, Args...> grad = prob.gradient<Args...>();
  RM::RiemannianMetric<DeviceVector, DeviceVector, double, Args...> metric = prob.metric<Args...>();
  RM::Retraction<DeviceVector, DeviceVector, Args...> retract = prob.retraction<Args...>();
  if constexpr (sizeof...(Args) == 0) {
    if (plain_retraction) retract = prob.plain_retraction();
  }
  if (wrap_objective) {
    auto tagged = f;
    f = [tagged](const DeviceVector &X, Args &...a) { return tagged(X, a...) + 1.0; };
  }
  mi_fusion_counters f0, f1;
  size_t c0 = 0, c1 = 0;
  ctx.synchronize();
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f0));
  MI355::check(mi_ctx_sync_count(ctx.get(), &c0));
  const auto t0 = Stopwatch::tick();
  auto r = RM::GradientDescent<DeviceVector, DeviceVector, double, Args...>(f, grad, metric, retract, x0, args..., gp);
  out->seconds = Stopwatch::tock(t0);
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

}  // namespace

extern "C" int hg_gd_so3n(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w,
                          const double *R0, size_t max_iterations, double gradient_tolerance, double alpha, double beta,
                          double sigma, size_t max_ls_iterations, int mode, double *x_out, double *f_out,
                          double *gradnorm_out, int *status_out, size_t *iterations_out, size_t cap,
                          double *objective_values, size_t *linesearch_iterations, GdOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    if (mode < 0 || mode > 3) throw std::invalid_argument("mode must be 0 ... 3");
    Context ctx(0);
    MI355::RotationAveraging prob(ctx, N, E, ei, ej, Rt, w);
    DeviceVector x0(ctx, R0, 9 * N);
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
    if (mode == 2) {
      DeviceVector cache(ctx, std::vector<double>(4, 2.0));
      r = gd_on<DeviceVector>(prob, ctx, x0, gp, false, false, out, cache);
    } else {
      r = gd_on(prob, ctx, x0, gp, mode == 1, mode == 3, out);
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
  } catch (const std::invalid_argument &e) {
    g_msg = e.what();
    return -1;
  } catch (const std::exception &e) {
    g_msg = e.what();
    return -2;
  }
  return 0;
}
