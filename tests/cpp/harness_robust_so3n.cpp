// harness_robust_so3n.cpp -- graduated non-convexity around Riemannian::TNT on MI355::RotationAveraging the way a client of
// the drop-in headers writes it: one L2 solve, then `rounds` rounds of reweight(R, {GemanMcClure, c sqrt(mu)}) + TNT with mu
// halved each round.  Every round is repeated on a FRESH RotationAveraging created from that round's downloaded weights and
// run from the same start: tests/test_gpu_so3n_robust_solve.py holds the two against each other.  TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNT.h"

using namespace Optimization;
namespace RM = Optimization::Riemannian;
using MI355::Context;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *hr_last_error() { return g_msg.c_str(); }

namespace {
struct Run {
  DeviceVector x;
  size_t outer = 0, inner = 0;
  int status = -1;
};
Run run_tnt(MI355::RotationAveraging &prob, const DeviceVector &R0) {
  RM::TNTParams<double> tp;
  tp.max_iterations = 100;
  tp.gradient_tolerance = 1e-9;
  tp.relative_decrease_tolerance = 0.0;
  tp.stepsize_tolerance = 0.0;
  tp.preconditioned_gradient_tolerance = 0.0;
  std::optional<RM::LinearOperator<DeviceVector, DeviceVector>> pc = prob.preconditioner();
  auto res = RM::TNT<DeviceVector, DeviceVector>(prob.objective(), prob.quadratic_model(), prob.metric(), prob.retraction(), R0,
                                                 pc, tp);
  Run r;
  r.x = res.x;
  r.outer = res.inner_iterations.size();
  for (size_t k : res.inner_iterations) r.inner += k;
  r.status = static_cast<int>(res.status);
  return r;
}
void put(const DeviceVector &v, double *dst) {
  const std::vector<double> h = v.to_host();
  std::memcpy(dst, h.data(), h.size() * sizeof(double));
}
}  // namespace

// R_l2: 9N; R_rounds, R_fresh: rounds x 9N; W: rounds x E; counts: rounds x 6 = {outer, inner, status} of the reweighted
// problem, then of the fresh one; outliers: rounds
extern "C" int hr_gnc_so3n(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w,
                           const double *R0, double c, double mu0, int rounds, double *R_l2, double *R_rounds, double *R_fresh,
                           double *W, long long *counts, long long *outliers) {
  try {
    Context ctx(0);
    MI355::RotationAveraging prob(ctx, N, E, ei, ej, Rt, w);
    Run cur = run_tnt(prob, DeviceVector(ctx, R0, 9 * N));
    put(cur.x, R_l2);
    double mu = mu0;
    for (int k = 0; k < rounds; ++k, mu *= .5) {
      const DeviceVector start = cur.x;
      const MI355::ReweightInfo info =
          prob.reweight(start, MI355::RobustKernel{MI355::RobustKernel::GemanMcClure, c * std::sqrt(mu)});
      outliers[k] = (long long)info.outliers;
      const std::vector<double> wk = prob.weights();
      std::memcpy(W + (size_t)k * E, wk.data(), E * sizeof(double));
      cur = run_tnt(prob, start);
      put(cur.x, R_rounds + (size_t)k * 9 * N);
      MI355::RotationAveraging fresh(ctx, N, E, ei, ej, Rt, wk.data());
      const Run f = run_tnt(fresh, DeviceVector(ctx, start.to_host().data(), 9 * N));
      put(f.x, R_fresh + (size_t)k * 9 * N);
      const long long row[6] = {(long long)cur.outer, (long long)cur.inner, cur.status,
                                (long long)f.outer, (long long)f.inner, f.status};
      std::memcpy(counts + 6 * k, row, sizeof(row));
    }
  } catch (const std::invalid_argument &e) {
    g_msg = e.what();
    return -1;
  } catch (const std::exception &e) {
    g_msg = e.what();
    return -2;
  }
  return 0;
}
