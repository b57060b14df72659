// harness_tnls_so3n.cpp -- Riemannian::TNLS on chordal rotation averaging over SO(3)^N as a nonlinear least-squares
// problem, F(R)_e = sqrt(w_e) (R_j - R_i Rt_e) in R^{9E}, the way a client of the drop-in headers writes it.  One templated
// driver, three modes:
//   0 (h)  this repository's TNLS.h on a plain host vector, with a plain-C++ restatement of F, dF, dF* and the retraction
//          written here (no device, no library call): the CPU truth of the runs below
//   1 (d)  MI355::DeviceVector with the tagged accessors of MI355::RotationAveraging (residual(), jacobian(), metric(),
//          residual_inner_product(), retraction(), gauss_newton_preconditioner()): every inner solve in the fused mi_lsqr
//   2 (g)  MI355::DeviceVector with the same device operators behind plain lambdas: the generic LSQR loop
// tests/test_cpu_so3n_nls.py and tests/test_gpu_so3n_nls.py hold the runs against each other and against
// tests/golden/tnls_so3n.json.  TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNLS.h"

using namespace Optimization;
namespace RM = Optimization::Riemannian;
namespace LA = Optimization::LinearAlgebra;
using MI355::Context;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *ht_last_error() { return g_msg.c_str(); }

namespace {

// Minimal host vector satisfying the implicit Vector concept; sequential dot (the HostVec of the other host harnesses)
struct HostVec {
  std::vector<double> d;
  HostVec() = default;
  explicit HostVec(size_t n) : d(n) {}
  HostVec(const double *p, size_t n) : d(p, p + n) {}
  size_t size() const { return d.size(); }
  double dot(const HostVec &o) const {
    double s = 0;
    for (size_t i = 0; i < d.size(); ++i) s += d[i] * o.d[i];
    return s;
  }
  HostVec &operator+=(const HostVec &o) {
    for (size_t i = 0; i < d.size(); ++i) d[i] += o.d[i];
    return *this;
  }
  HostVec &operator-=(const HostVec &o) {
    for (size_t i = 0; i < d.size(); ++i) d[i] -= o.d[i];
    return *this;
  }
  HostVec &operator*=(double a) {
    for (auto &x : d) x *= a;
    return *this;
  }
  HostVec &operator/=(double a) {
    for (auto &x : d) x /= a;
    return *this;
  }
};
[[maybe_unused]] HostVec operator*(double a, const HostVec &v) {
  HostVec r(v.size());
  for (size_t i = 0; i < v.size(); ++i) r.d[i] = a * v.d[i];
  return r;
}
[[maybe_unused]] HostVec operator/(const HostVec &v, double a) {
  HostVec r(v.size());
  for (size_t i = 0; i < v.size(); ++i) r.d[i] = v.d[i] / a;
  return r;
}
[[maybe_unused]] HostVec operator+(const HostVec &a, const HostVec &b) {
  HostVec r(a.size());
  for (size_t i = 0; i < a.size(); ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
[[maybe_unused]] HostVec operator-(const HostVec &a, const HostVec &b) {
  HostVec r(a.size());
  for (size_t i = 0; i < a.size(); ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
[[maybe_unused]] HostVec operator-(const HostVec &a) {
  HostVec r(a.size());
  for (size_t i = 0; i < a.size(); ++i) r.d[i] = -a.d[i];
  return r;
}

// ---- the problem in plain C++ (row-major 3x3 blocks; hat / vee of optimization_amd/csrc/so3.hip) ------------------------
void mul(const double *A, const double *B, double *C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
void mul_at(const double *A, const double *B, double *C) {  // A' B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
void mul_bt(const double *A, const double *B, double *C) {  // A B'
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1] + A[i * 3 + 2] * B[j * 3 + 2];
}
void hat(const double *x, double *K) {
  K[0] = 0; K[1] = -x[2]; K[2] = x[1];
  K[3] = x[2]; K[4] = 0; K[5] = -x[0];
  K[6] = -x[1]; K[7] = x[0]; K[8] = 0;
}
void vee(const double *M, double *o) {
  o[0] = M[7] - M[5];
  o[1] = M[2] - M[6];
  o[2] = M[3] - M[1];
}

struct HostProblem {
  size_t N, E;
  const int32_t *ei, *ej;
  const double *Rt, *w;
  HostVec F(const HostVec &R) const {
    HostVec out(9 * E);
    for (size_t e = 0; e < E; ++e) {
      const double *Ri = &R.d[9 * (size_t)ei[e]], *Rj = &R.d[9 * (size_t)ej[e]];
      double RiS[9];
      mul(Ri, Rt + 9 * e, RiS);
      const double sw = std::sqrt(w[e]);
      for (int c = 0; c < 9; ++c) out.d[9 * e + c] = sw * (Rj[c] - RiS[c]);
    }
    return out;
  }
  HostVec dF(const HostVec &R, const HostVec &xi) const {
    HostVec out(9 * E);
    for (size_t e = 0; e < E; ++e) {
      const size_t i = (size_t)ei[e], j = (size_t)ej[e];
      double Ki[9], Kj[9], A[9], B[9], BS[9];
      hat(&xi.d[3 * i], Ki);
      hat(&xi.d[3 * j], Kj);
      mul(&R.d[9 * j], Kj, A);
      mul(&R.d[9 * i], Ki, B);
      mul(B, Rt + 9 * e, BS);
      const double sw = std::sqrt(w[e]);
      for (int c = 0; c < 9; ++c) out.d[9 * e + c] = sw * (A[c] - BS[c]);
    }
    return out;
  }
  HostVec dFt(const HostVec &R, const HostVec &Y) const {
    HostVec out(3 * N);
    for (auto &v : out.d) v = 0;
    for (size_t e = 0; e < E; ++e) {
      const size_t i = (size_t)ei[e], j = (size_t)ej[e];
      const double sw = std::sqrt(w[e]);
      double T[9], U[9], o[3];
      mul_at(&R.d[9 * i], &Y.d[9 * e], T);  // R_i' Y_e
      mul_bt(T, Rt + 9 * e, U);             // ... Rt_e'
      vee(U, o);
      for (int c = 0; c < 3; ++c) out.d[3 * i + c] -= sw * o[c];
      mul_at(&R.d[9 * j], &Y.d[9 * e], T);
      vee(T, o);
      for (int c = 0; c < 3; ++c) out.d[3 * j + c] += sw * o[c];
    }
    return out;
  }
  // Y_i = R_i exp(hat(xi_i)): Rodrigues with the series below |xi| = 1e-4
  HostVec retract(const HostVec &R, const HostVec &xi) const {
    HostVec Y(9 * N);
    for (size_t i = 0; i < N; ++i) {
      const double *x = &xi.d[3 * i];
      const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], th = std::sqrt(th2);
      double a, b;
      if (th < 1e-4) {
        a = 1 - th2 / 6 + th2 * th2 / 120;
        b = .5 - th2 / 24 + th2 * th2 / 720;
      } else {
        a = std::sin(th) / th;
        b = (1 - std::cos(th)) / th2;
      }
      double K[9], K2[9], Ex[9];
      hat(x, K);
      mul(K, K, K2);
      for (int c = 0; c < 9; ++c) Ex[c] = a * K[c] + b * K2[c];
      Ex[0] += 1; Ex[4] += 1; Ex[8] += 1;
      mul(&R.d[9 * i], Ex, &Y.d[9 * i]);
    }
    return Y;
  }
  // diag(1 / sqrt(2 degw_i)), each entry three times (1 for a node without weight)
  std::vector<double> gn_scaling() const {
    std::vector<double> degw(N, 0.0), d(3 * N);
    for (size_t e = 0; e < E; ++e) {
      degw[(size_t)ei[e]] += w[e];
      degw[(size_t)ej[e]] += w[e];
    }
    for (size_t i = 0; i < N; ++i) d[3 * i] = d[3 * i + 1] = d[3 * i + 2] = degw[i] > 0 ? 1.0 / std::sqrt(2 * degw[i]) : 1.0;
    return d;
  }
};

struct TnlsOut {  // plain data, mirrored by ctypes in tests/harness_tnls_so3n_py.py
  mi_fusion_counters fusion;  // of the run's own context, over the optimizer call (zero in mode 0)
  int status;
  size_t outer;               // outer iterations that ran an inner solve
  double f, gradnorm;         // |F(x)|, |grad L(x)| at the final point
};

template <typename V>
void store(const RM::TNLSResult<V, double> &r, const std::vector<double> &x, size_t cap, double *x_out, size_t *inner,
           double *rho, double *radius, double *fnorms, TnlsOut *out) {
  std::memcpy(x_out, x.data(), x.size() * sizeof(double));
  out->status = static_cast<int>(r.status);
  out->outer = r.inner_iterations.size();
  out->f = r.f;
  out->gradnorm = r.gradfx_norm;
  for (size_t k = 0; k < r.inner_iterations.size() && k < cap; ++k) {
    inner[k] = r.inner_iterations[k];
    rho[k] = r.rho[k];
    radius[k] = r.trust_region_radius[k];
    fnorms[k] = r.objective_values[k];
  }
}

}  // namespace

// mode: 0 host, 1 device tagged, 2 device behind plain lambdas.  kappa_fgr: the cap of LSQR's btol (TNLSParams).
// inner / rho / radius / fnorms: per outer iteration k < cap -- LSQR passes, gain ratio, radius and |F| at its start.
extern "C" int ht_tnls_so3n(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w,
                            const double *R0, int mode, int with_precon, double Delta0, double kappa_fgr,
                            double gradient_tolerance, size_t max_iterations, size_t max_lsqr_iterations, size_t cap,
                            double *x_out, size_t *inner, double *rho, double *radius, double *fnorms, TnlsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    if (mode < 0 || mode > 2) throw std::invalid_argument("mode must be 0, 1 or 2");
    RM::TNLSParams<double> p;
    p.relative_decrease_tolerance = 0;
    p.stepsize_tolerance = 0;
    p.root_tolerance = 0;
    p.gradient_tolerance = gradient_tolerance;
    p.max_iterations = max_iterations;
    p.max_LSQR_iterations = max_lsqr_iterations;
    p.Delta0 = Delta0;
    p.kappa_fgr = kappa_fgr;
    if (mode == 0) {
      const HostProblem hp{N, E, ei, ej, Rt, w};
      const std::vector<double> dg = hp.gn_scaling();
      RM::Mapping<HostVec, HostVec> F = [&](const HostVec &R) { return hp.F(R); };
      RM::JacobianPairFunction<HostVec, HostVec, HostVec> J = [&](const HostVec &) {
        RM::Jacobian<HostVec, HostVec, HostVec> dF = [&](const HostVec &R, const HostVec &v) { return hp.dF(R, v); };
        RM::JacobianAdjoint<HostVec, HostVec, HostVec> dFt = [&](const HostVec &R, const HostVec &y) { return hp.dFt(R, y); };
        return std::make_pair(dF, dFt);
      };
      RM::RiemannianMetric<HostVec, HostVec, double> metric = [](const HostVec &, const HostVec &a, const HostVec &b) { return a.dot(b); };
      LA::InnerProduct<HostVec, double> ipY = [](const HostVec &a, const HostVec &b) { return a.dot(b); };
      RM::Retraction<HostVec, HostVec> retract = [&](const HostVec &R, const HostVec &v) { return hp.retract(R, v); };
      RM::LinearOperator<HostVec, HostVec> M = [&](const HostVec &, const HostVec &v) {
        HostVec r(v.size());
        for (size_t i = 0; i < v.size(); ++i) r.d[i] = dg[i] * v.d[i];
        return r;
      };
      std::optional<RM::TNLSPreconditioner<HostVec, HostVec>> precon;
      if (with_precon) precon = std::make_pair(M, M);
      const HostVec x0(R0, 9 * N);
      const auto r = RM::TNLS<HostVec, HostVec, HostVec, double>(F, J, metric, ipY, retract, x0, precon, p);
      store(r, r.x.d, cap, x_out, inner, rho, radius, fnorms, out);
      return 0;
    }
    Context ctx(0);
    MI355::RotationAveraging prob(ctx, N, E, ei, ej, Rt, w);
    RM::Mapping<DeviceVector, DeviceVector> F = prob.residual();
    RM::JacobianPairFunction<DeviceVector, DeviceVector, DeviceVector> J = prob.jacobian();
    RM::RiemannianMetric<DeviceVector, DeviceVector, double> metric = prob.metric();
    LA::InnerProduct<DeviceVector, double> ipY = prob.residual_inner_product();
    RM::Retraction<DeviceVector, DeviceVector> retract = prob.retraction();
    std::optional<RM::TNLSPreconditioner<DeviceVector, DeviceVector>> precon;
    if (with_precon) precon = prob.gauss_newton_preconditioner();
    if (mode == 2) {
      // the same device work, the tags lost: LSQR must run its generic loop
      auto tJ = J;
      J = [tJ](const DeviceVector &R) {
        auto pr = tJ(R);
        auto a = pr.first;
        auto at = pr.second;
        RM::Jacobian<DeviceVector, DeviceVector, DeviceVector> dF = [a](const DeviceVector &X, const DeviceVector &v) { return a(X, v); };
        RM::JacobianAdjoint<DeviceVector, DeviceVector, DeviceVector> dFt = [at](const DeviceVector &X, const DeviceVector &y) { return at(X, y); };
        return std::make_pair(dF, dFt);
      };
      metric = [](const DeviceVector &, const DeviceVector &a, const DeviceVector &b) { return a.dot(b); };
      ipY = [](const DeviceVector &a, const DeviceVector &b) { return a.dot(b); };
      if (with_precon) {
        auto m = precon->first;
        RM::LinearOperator<DeviceVector, DeviceVector> M = [m](const DeviceVector &X, const DeviceVector &v) { return m(X, v); };
        precon = std::make_pair(M, M);
      }
    }
    DeviceVector x0(ctx, R0, 9 * N);
    mi_fusion_counters f0, f1;
    ctx.synchronize();
    MI355::check(mi_ctx_fusion_counters(ctx.get(), &f0));
    const auto r = RM::TNLS<DeviceVector, DeviceVector, DeviceVector, double>(F, J, metric, ipY, retract, x0, precon, p);
    MI355::check(mi_ctx_fusion_counters(ctx.get(), &f1));
    store(r, r.x.to_host(), cap, x_out, inner, rho, radius, fnorms, out);
    out->fusion.fused_stpcg_solves = f1.fused_stpcg_solves - f0.fused_stpcg_solves;
    out->fusion.generic_stpcg_solves = f1.generic_stpcg_solves - f0.generic_stpcg_solves;
    out->fusion.fused_lsqr_solves = f1.fused_lsqr_solves - f0.fused_lsqr_solves;
    out->fusion.generic_lsqr_solves = f1.generic_lsqr_solves - f0.generic_lsqr_solves;
    out->fusion.fused_trial_steps = f1.fused_trial_steps - f0.fused_trial_steps;
    out->fusion.generic_trial_steps = f1.generic_trial_steps - f0.generic_trial_steps;
    out->fusion.generic_inner_products = f1.generic_inner_products - f0.generic_inner_products;
  } catch (const std::invalid_argument &e) {
    g_msg = e.what();
    return -1;
  } catch (const std::exception &e) {
    g_msg = e.what();
    return -2;
  }
  return 0;
}
