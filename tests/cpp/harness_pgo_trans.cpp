// harness_pgo_trans.cpp -- MI355::TranslationRecovery the way a client of the drop-in headers calls it: solve(), and the
// client's own LinearAlgebra::STPCG call with laplacian() and jacobi() on g = -rhs(R) (the call solve() makes through the C
// ABI: a radius that never binds, theta = 0, kappa_fgr = tol).  The fusion counters around each of the two are reported:
// both must be one fused solve with no generic inner product.  tests/test_gpu_pgo_trans.py compares both iterates with the
// C-ABI result bit for bit.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/LinearAlgebra/IterativeSolvers.h"
#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/PoseGraph.h"

using namespace Optimization;
namespace LA = Optimization::LinearAlgebra;
using MI355::Context;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *hp_last_error() { return g_msg.c_str(); }

struct PgoOut {  // plain data, mirrored by ctypes in tests/harness_pgo_trans_py.py
  double objective, relative_residual, max_residual, residuals_objective, residuals_max, client_M_norm;
  size_t iterations, client_iterations;
  unsigned long long solve_fused, solve_generic, solve_inner_products, client_fused, client_generic, client_inner_products;
  int exit_reason;
};

extern "C" int hp_pgo_trans(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *tt, const double *tau,
                            long long anchor, const double *R_host, double tol, size_t max_iterations, double *t_solve_out,
                            double *t_client_out, double *b_out, double *r_out, PgoOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    MI355::TranslationRecovery rec(ctx, N, E, ei, ej, tt, tau, anchor);
    const DeviceVector R(ctx, R_host, 9 * N);
    mi_fusion_counters fc;
    // (1) solve()
    MI355::check(mi_ctx_fusion_counters_reset(ctx.get()));
    MI355::TranslationParams tp;
    tp.tol = tol;
    tp.max_iterations = max_iterations;
    const MI355::TranslationResult s = rec.solve(R, tp);
    MI355::check(mi_ctx_fusion_counters(ctx.get(), &fc));
    out->solve_fused = fc.fused_stpcg_solves, out->solve_generic = fc.generic_stpcg_solves;
    out->solve_inner_products = fc.generic_inner_products;
    out->objective = s.objective, out->relative_residual = s.relative_residual, out->max_residual = s.max_residual;
    out->iterations = s.iterations, out->exit_reason = s.exit;
    const std::vector<double> ts = s.t.to_host();
    std::memcpy(t_solve_out, ts.data(), ts.size() * sizeof(double));
    // (2) the client's own STPCG call
    const DeviceVector b = rec.rhs(R);
    const std::vector<double> bh = b.to_host();
    std::memcpy(b_out, bh.data(), bh.size() * sizeof(double));
    const DeviceVector g = -1.0 * b;
    const LA::SymmetricLinearOperator<DeviceVector> L = rec.laplacian();
    const LA::InnerProduct<DeviceVector> ip = MI355::FrobeniusInnerProduct{};
    const std::optional<LA::STPCGPreconditioner<DeviceVector, std::nullptr_t>> P = rec.jacobi();
    MI355::check(mi_ctx_fusion_counters_reset(ctx.get()));
    double mn = 0;
    size_t it = 0;
    const DeviceVector tc = LA::STPCG<DeviceVector, std::nullptr_t>(g, L, ip, mn, it, 1e150, max_iterations, tol, 0.0, P);
    MI355::check(mi_ctx_fusion_counters(ctx.get(), &fc));
    out->client_fused = fc.fused_stpcg_solves, out->client_generic = fc.generic_stpcg_solves;
    out->client_inner_products = fc.generic_inner_products;
    out->client_iterations = it, out->client_M_norm = mn;
    const std::vector<double> th = tc.to_host();
    std::memcpy(t_client_out, th.data(), th.size() * sizeof(double));
    // (3) residuals() at the solve's iterate
    const MI355::TranslationResiduals rr = rec.residuals(R, s.t);
    out->residuals_objective = rr.objective, out->residuals_max = rr.max_residual;
    const std::vector<double> rh = rr.r.to_host();
    if (!rh.empty()) std::memcpy(r_out, rh.data(), rh.size() * sizeof(double));
  } catch (const std::invalid_argument &e) {
    g_msg = e.what();
    return -1;
  } catch (const std::exception &e) {
    g_msg = e.what();
    return -2;
  }
  return 0;
}
