// harness_spectral_so3n.cpp -- MI355::RotationAveraging::spectral_initialization (the three lowest eigenvectors of the
// connection Laplacian through the device LOBPCG, rounded to SO(3)^N) the way a client of the drop-in headers calls it,
// and with run_tnt what follows from it: Riemannian::TNT from the spectral point (block-Jacobi preconditioner, stop on the
// gradient tolerance) and certify() at what TNT reaches.  tests/test_gpu_so3n_spectral.py holds the runs against numpy.
// TEST INFRASTRUCTURE ONLY.
#include <chrono>
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
extern "C" const char *hs_last_error() { return g_msg.c_str(); }

struct SpectralOut {  // plain data, mirrored by ctypes in tests/harness_spectral_so3n_py.py
  double eigenvalues[3];
  double f, lower_bound, min_separation;
  double f_final, tnt_gradnorm, cert_lambda_min, cert_lambda_min_safe, cert_eta;
  double seconds_spectral, seconds_tnt;  // wall clock around spectral_initialization() and around the TNT call
  size_t iterations, degenerate, tnt_iterations, cert_iterations;
  int converged, flipped, has_eigenvectors, tnt_status, certified, cert_converged;
};

extern "C" int hs_spectral_so3n(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w,
                                size_t nx, double tau, size_t max_iterations, int precondition, int run_tnt,
                                double tnt_gradient_tolerance, size_t cert_max_iterations, double *R0_out,
                                double *eigenvectors_out, double *R_final_out, SpectralOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    MI355::RotationAveraging prob(ctx, N, E, ei, ej, Rt, w);
    MI355::SpectralParams sp;
    sp.nx = nx;
    sp.tau = tau;
    sp.max_iterations = max_iterations;
    sp.precondition = precondition != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const MI355::SpectralResult s = prob.spectral_initialization(sp);
    out->seconds_spectral = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < 3; ++i) out->eigenvalues[i] = s.eigenvalues[i];
    out->f = s.f;
    out->lower_bound = s.lower_bound;
    out->min_separation = s.min_separation;
    out->iterations = s.iterations;
    out->degenerate = s.degenerate;
    out->converged = s.converged ? 1 : 0;
    out->flipped = s.flipped ? 1 : 0;
    out->has_eigenvectors = s.eigenvectors.empty() ? 0 : 1;
    const std::vector<double> r0 = s.R.to_host();
    std::memcpy(R0_out, r0.data(), r0.size() * sizeof(double));
    if (!s.eigenvectors.empty()) {
      const std::vector<double> v = s.eigenvectors.to_host();
      std::memcpy(eigenvectors_out, v.data(), v.size() * sizeof(double));
    }
    out->tnt_status = -1;
    if (run_tnt) {
      RM::TNTParams<double> tp;
      tp.max_iterations = 200;
      tp.gradient_tolerance = tnt_gradient_tolerance;
      tp.relative_decrease_tolerance = 0.0;
      tp.stepsize_tolerance = 0.0;
      tp.preconditioned_gradient_tolerance = 0.0;
      std::optional<RM::LinearOperator<DeviceVector, DeviceVector>> pc = prob.preconditioner();
      const auto t1 = std::chrono::steady_clock::now();
      auto res = RM::TNT<DeviceVector, DeviceVector>(prob.objective(), prob.quadratic_model(), prob.metric(),
                                                     prob.retraction(), s.R, pc, tp);
      out->seconds_tnt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
      out->tnt_gradnorm = res.gradfx_norm;
      out->tnt_iterations = res.inner_iterations.size();
      out->tnt_status = static_cast<int>(res.status);
      out->f_final = res.f;
      if (cert_max_iterations > 0) {  // (0: no certificate -- tools/bench_spectral.py times the first two steps only)
        MI355::CertifyParams cp;
        cp.max_iterations = cert_max_iterations;
        const MI355::CertifyResult c = prob.certify(res.x, cp);
        out->f_final = c.f;
        out->cert_lambda_min = c.lambda_min;
        out->cert_lambda_min_safe = c.lambda_min_safe;
        out->cert_eta = c.eta;
        out->cert_iterations = c.iterations;
        out->cert_converged = c.converged ? 1 : 0;
        out->certified = c.certified ? 1 : 0;
      }
      const std::vector<double> x = res.x.to_host();
      std::memcpy(R_final_out, x.data(), x.size() * sizeof(double));
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
