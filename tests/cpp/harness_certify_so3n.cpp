// harness_certify_so3n.cpp -- MI355::RotationAveraging::certify (the global-optimality certificate of a point of SO(3)^N
// through the device LOBPCG) the way a client of the drop-in headers calls it.  The point is R0 itself or, with run_tnt,
// what Riemannian::TNT reaches from R0 (block-Jacobi preconditioner, stop on the gradient tolerance).  op_mode:
//   0  prob.certify(R): the tagged CertificateOperator inside the SymmetricLinearOperator
//   1  the same operator behind a plain lambda (certify_with): LOBPCG must take the same path and the same iterations
//   2  mode 0, and the eigenvector's residual re-formed through the operator's PanelBlocks form (one block) into
//      blocks_residual: |S x - lambda x|
// tests/test_gpu_so3n_certificate.py holds the runs against the closed forms and against numpy.  TEST INFRASTRUCTURE ONLY.
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
namespace LA = Optimization::LinearAlgebra;
using MI355::Context;
using MI355::DeviceMatrix;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *hc_last_error() { return g_msg.c_str(); }

struct CertOut {  // plain data, mirrored by ctypes in tests/harness_certify_so3n_py.py
  double lambda_min, lambda_min_safe, f, lower_bound, stationarity, norm_estimate, eta;
  double tnt_gradnorm, blocks_residual;
  size_t iterations, tnt_iterations;
  int converged, certified, tnt_status;
};

extern "C" int hc_certify_so3n(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w,
                               const double *R0, int run_tnt, double tnt_gradient_tolerance, size_t nx, double tau,
                               size_t max_iterations, double eta, int op_mode, double *R_out, double *eigenvector_out,
                               CertOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    if (op_mode < 0 || op_mode > 2) throw std::invalid_argument("op_mode must be 0 ... 2");
    Context ctx(0);
    MI355::RotationAveraging prob(ctx, N, E, ei, ej, Rt, w);
    DeviceVector R(ctx, R0, 9 * N);
    out->tnt_status = -1;
    if (run_tnt) {
      RM::TNTParams<double> tp;
      tp.max_iterations = 200;
      tp.gradient_tolerance = tnt_gradient_tolerance;
      tp.relative_decrease_tolerance = 0.0;
      tp.stepsize_tolerance = 0.0;
      tp.preconditioned_gradient_tolerance = 0.0;
      std::optional<RM::LinearOperator<DeviceVector, DeviceVector>> pc = prob.preconditioner();
      auto res = RM::TNT<DeviceVector, DeviceVector>(prob.objective(), prob.quadratic_model(), prob.metric(),
                                                     prob.retraction(), R, pc, tp);
      out->tnt_gradnorm = res.gradfx_norm;
      out->tnt_iterations = res.inner_iterations.size();
      out->tnt_status = static_cast<int>(res.status);
      R = res.x;
    }
    MI355::CertifyParams cp;
    cp.nx = nx;
    cp.tau = tau;
    cp.max_iterations = max_iterations;
    cp.eta = eta;
    MI355::CertifyResult r;
    if (op_mode == 1) {
      const LA::SymmetricLinearOperator<DeviceMatrix> tagged = prob.certificate_operator(R);
      const MI355::CertificateOperator info = *tagged.target<MI355::CertificateOperator>();
      const LA::SymmetricLinearOperator<DeviceMatrix> plain = [info](const DeviceMatrix &X) { return info(X); };
      r = prob.certify_with(plain, info, cp);
    } else {
      r = prob.certify(R, cp);
    }
    out->lambda_min = r.lambda_min;
    out->lambda_min_safe = r.lambda_min_safe;
    out->f = r.f;
    out->lower_bound = r.lower_bound;
    out->stationarity = r.stationarity;
    out->norm_estimate = r.norm_estimate;
    out->eta = r.eta;
    out->iterations = r.iterations;
    out->converged = r.converged ? 1 : 0;
    out->certified = r.certified ? 1 : 0;
    out->blocks_residual = -1;
    if (op_mode == 2 && !r.eigenvector.empty()) {
      // (certify() bound the problem's certificate to R last: a fresh operator is the same matrix)
      const auto A = prob.certificate_operator(R);
      MI355::PanelBlocks blk;
      blk.add(r.eigenvector.leftCols(1));
      const DeviceMatrix Sx = (*A.target<MI355::CertificateOperator>())(blk);
      const std::vector<double> sx = Sx.to_host(), x = r.eigenvector.to_host();
      double s = 0;
      for (size_t i = 0; i < x.size(); ++i) s += (sx[i] - r.lambda_min * x[i]) * (sx[i] - r.lambda_min * x[i]);
      out->blocks_residual = std::sqrt(s);
    }
    const std::vector<double> x = R.to_host();
    std::memcpy(R_out, x.data(), x.size() * sizeof(double));
    if (!r.eigenvector.empty()) {
      const std::vector<double> v = r.eigenvector.to_host();
      std::memcpy(eigenvector_out, v.data(), v.size() * sizeof(double));
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
