// Optimization/MI355/PoseGraph.h -- pose graphs on the device: TranslationRecovery (the positions for fixed rotations) and
// PoseGraph (rotations and positions refined together on SE(3)^N, below).
// With the rotations R fixed (the 9N point of MI355::RotationAveraging: what spectral_initialization(), TNT, TNLS or
// GradientDescent return) the positions of the edges e = (i -> j) with relative translations tt_e and weights tau_e solve
//     min_t  1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2    <=>    L_a t = b(R),   t_anchor = 0,
// the second stage of chordal initialisation.  TranslationRecovery owns the anchored graph Laplacian L_a (a device CSR
// matrix on the N x 3 row-major field), its Jacobi preconditioner and the two passes that depend on R:
//   rhs(R)            b(R), 3N
//   laplacian()       L_a as a tagged SymmetricLinearOperator<DeviceVector>   } a client's own LinearAlgebra::STPCG call
//   jacobi()          its tagged STPCGPreconditioner                          } with them takes the fused device path
//   residuals(R, t)   r_e = t_j - t_i - R_i tt_e per edge, the objective and max_e |r_e|
//   solve(R)          rhs -> fused PCG from t = 0 -> residual pass
// Kernels: optimization_amd/csrc/pgo_trans.hip; C ABI: mi355opt.h section (7b).  Single-context only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "Optimization/LinearAlgebra/Concepts.h"
#include "Optimization/LinearAlgebra/IterativeSolvers.h"
#include "Optimization/MI355/Device.h"
#include "Optimization/Riemannian/Concepts.h"
#include "Optimization/Riemannian/TNT.h"

namespace Optimization {
namespace MI355 {

struct TranslationParams {
  double tol = 1e-10;            // stop at sqrt(<r,v>) <= tol sqrt(<r0,v0>) (v = the Jacobi-preconditioned residual)
  size_t max_iterations = 1000;
};
struct TranslationResult {
  DeviceVector t;                // 3N: the positions, t[anchor] = 0
  size_t iterations = 0;
  int exit = 0;                  // MI_STPCG_EXIT_*: RESIDUAL is convergence
  double objective = 0;          // 1/2 sum_e tau_e |r_e|^2 at (R, t)
  double relative_residual = 0;  // |L_a t - b| / |b| from one plain application after the solve
  double max_residual = 0;       // max_e |r_e|
};
struct TranslationResiduals {
  DeviceVector r;                // 3E: r_e in the caller's edge order
  double objective = 0, max_residual = 0;
};

class TranslationRecovery {
 public:
  using Vector = DeviceVector;

  TranslationRecovery(const Context &ctx, size_t N, size_t n_edges, const int32_t *ei, const int32_t *ej, const double *tt,
                      const double *tau, long long anchor = 0)
      : ctx_(ctx), N_(N), E_(n_edges) {
    check(mi_pgo_trans_create(ctx_.get(), N, n_edges, ei, ej, tt, tau, anchor, &T_));
  }
  TranslationRecovery(const TranslationRecovery &) = delete;
  TranslationRecovery &operator=(const TranslationRecovery &) = delete;
  ~TranslationRecovery() {
    if (T_) mi_pgo_trans_destroy(T_);
  }

  size_t poses() const { return N_; }
  size_t edges() const { return E_; }
  mi_pgo_trans *handle() const { return T_; }

  Vector rhs(const Vector &R) const {
    Vector b(ctx_, 3 * N_);
    check(mi_pgo_trans_rhs(T_, R.handle(), b.handle()));
    return b;
  }
  // tagged (found again with std::function::target): STPCG(g, laplacian(), FrobeniusInnerProduct{}, ..., jacobi()) is one
  // fused device solve.  Both live as long as this object.
  template <typename... Args>
  LinearAlgebra::SymmetricLinearOperator<Vector, Args...> laplacian() const {
    mi_op *L = nullptr;
    check(mi_pgo_trans_operator(T_, &L, nullptr));
    return DeviceOperator{L};
  }
  template <typename Multiplier = std::nullptr_t, typename... Args>
  LinearAlgebra::STPCGPreconditioner<Vector, Multiplier, Args...> jacobi() const {
    mi_precon *P = nullptr;
    check(mi_pgo_trans_operator(T_, nullptr, &P));
    return DeviceSTPCGPreconditioner<Multiplier>{P};
  }
  // with_vector = false: only the two numbers (nothing written)
  TranslationResiduals residuals(const Vector &R, const Vector &t, bool with_vector = true) const {
    TranslationResiduals out;
    if (with_vector) out.r = Vector(ctx_, 3 * E_);
    double s[2];
    check(mi_pgo_trans_residual(T_, R.handle(), t.handle(), with_vector ? out.r.handle() : nullptr, s));
    out.objective = s[0];
    out.max_residual = s[1];
    return out;
  }
  TranslationResult solve(const Vector &R, const TranslationParams &params = TranslationParams()) const {
    TranslationResult out;
    out.t = Vector(ctx_, 3 * N_);
    mi_pgo_trans_info info;
    check(mi_pgo_trans_solve(T_, R.handle(), params.tol, params.max_iterations, out.t.handle(), &info));
    out.iterations = info.iterations;
    out.exit = info.exit_reason;
    out.objective = info.objective;
    out.relative_residual = info.relative_residual;
    out.max_residual = info.max_residual;
    return out;
  }

 private:
  Context ctx_;
  size_t N_, E_;
  mi_pgo_trans *T_ = nullptr;
};

// Joint refinement on SE(3)^N:
//     f(R, t) = 1/2 sum_e kappa_e | R_j - R_i Rt_e |_F^2  +  1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2,   e = (i -> j)
// in the shape the reference's templates expect.  Variable = 12N doubles [R | t] (the 9N point of RotationAveraging, then the
// 3N positions of TranslationRecovery: pack / rotations / translations), Tangent = 6N doubles, node-major [xi_i, delta_i],
// metric = coordinate dot, retraction R_i exp(hat xi_i), t_i + delta_i, preconditioner = 3x3 block-Jacobi over the 2N
// diagonal blocks of the Hessian.  Every accessor names this object as owner, so Riemannian::TNT runs its inner solve in
// the fused mi_stpcg and its trial step through mi_pgo_trial, one read-back per outer iteration.  No gauge is fixed.
// Kernels: optimization_amd/csrc/pgo.hip; C ABI: mi355opt.h section (7c).  Single-context only.
// A window of a DeviceVector that shares its storage (mi_vec_view), for as long as this object lives; it must not outlive
// the vector it was taken from.  Converts to const DeviceVector &: what RotationAveraging / TranslationRecovery take.
class DeviceVectorView {
 public:
  DeviceVectorView(const DeviceVector &base, size_t offset, size_t n) {
    check(mi_vec_view(base.handle(), offset, n, &v_));
    d_ = DeviceVector::view(base.context(), v_);
  }
  DeviceVectorView(DeviceVectorView &&o) noexcept : v_(o.v_), d_(std::move(o.d_)) { o.v_ = nullptr; }
  DeviceVectorView(const DeviceVectorView &) = delete;
  DeviceVectorView &operator=(const DeviceVectorView &) = delete;
  ~DeviceVectorView() {
    d_ = DeviceVector();
    if (v_) mi_vec_destroy(v_);
  }
  operator const DeviceVector &() const { return d_; }
  const DeviceVector &vector() const { return d_; }
  mi_vec *handle() const { return v_; }
  // writes THROUGH the view (DeviceVector's own assignment would rebind the wrapper to fresh storage)
  void assign(const DeviceVector &src) { check(mi_vec_copy(v_, src.handle())); }

 private:
  mi_vec *v_ = nullptr;
  DeviceVector d_;
};

struct PoseGraphResult {
  DeviceVector x;                  // 12N: the refined point
  double f = 0;                    // the objective there
  double gradient_norm = 0;
  size_t outer_iterations = 0;
  size_t inner_iterations = 0;     // summed over the outer iterations
  Riemannian::TNTStatus status = Riemannian::TNTStatus::IterationLimit;
};

class PoseGraph {
 public:
  using Vector = DeviceVector;

  PoseGraph(const Context &ctx, size_t N, size_t n_edges, const int32_t *ei, const int32_t *ej, const double *Rt,
            const double *tt, const double *kappa, const double *tau)
      : ctx_(ctx), N_(N), E_(n_edges) {
    check(mi_pgo_create(ctx_.get(), N, n_edges, ei, ej, Rt, tt, kappa, tau, &prob_));
  }
  PoseGraph(const PoseGraph &) = delete;
  PoseGraph &operator=(const PoseGraph &) = delete;
  ~PoseGraph() {
    if (prob_) mi_pgo_destroy(prob_);
  }

  size_t poses() const { return N_; }
  size_t edges() const { return E_; }
  mi_pgo *handle() const { return prob_; }

  // x = [R | t] (one copy of each half), and the halves of a point as views that share its storage: what
  // RotationAveraging / TranslationRecovery take without a copy; assign() through one lands in x
  Vector pack(const Vector &R, const Vector &t) const {
    Vector x(ctx_, 12 * N_);
    rotations(x).assign(R);
    translations(x).assign(t);
    return x;
  }
  DeviceVectorView rotations(const Vector &x) const { return DeviceVectorView(x, 0, 9 * N_); }
  DeviceVectorView translations(const Vector &x) const { return DeviceVectorView(x, 9 * N_, 3 * N_); }

  template <typename... Args>
  Objective<Vector, double, Args...> objective() {
    return DeviceObjective{this, [this](const Vector &x) {
                             double f = 0;
                             check(mi_pgo_objective(prob_, x.handle(), &f));
                             return f;
                           }};
  }
  // the gradient and the Hessian assembled at x; also refreshes the block-Jacobi preconditioner of preconditioner()
  template <typename... Args>
  Riemannian::QuadraticModel<Vector, Vector, Args...> quadratic_model() {
    return [this](const Vector &x, Vector &grad, Riemannian::LinearOperator<Vector, Vector, Args...> &Hess, Args &...) {
      if (grad.empty() || grad.size() != 6 * N_) grad = Vector(ctx_, 6 * N_);
      mi_op *op = nullptr;
      check(mi_pgo_model(prob_, x.handle(), grad.handle(), &op, &bj_));
      Hess = DeviceHessian{op, this};
    };
  }
  template <typename... Args>
  Riemannian::RiemannianMetric<Vector, Vector, double, Args...> metric() {
    return FrobeniusMetric{};
  }
  // tagged: TNT evaluates a whole trial step through mi_pgo_trial.  `armijo` stays empty: GradientDescent runs its
  // statement sequence on these callables.
  template <typename... Args>
  Riemannian::Retraction<Vector, Vector, Args...> retraction() {
    DeviceTrialRetraction r;
    r.owner = this;
    r.retract = [this](const Vector &x, const Vector &eta) { return retract(x, eta); };
    r.trial = [this](const Vector &x, const Vector &h, const Vector &g, bool with_precon) {
      DeviceTrialRetraction::Trial t;
      t.x_trial = Vector::like(x);
      double out[6];
      check(mi_pgo_trial(prob_, x.handle(), h.handle(), g.handle(), with_precon ? 1 : 0, t.x_trial.handle(), out));
      t.f_trial = out[0];
      t.hh = out[1];
      t.gh = out[2];
      t.hHh = out[3];
      t.grad_trial_sqnorm = out[4];
      t.precon_grad_trial_sqnorm = out[5];
      return t;
    };
    return r;
  }
  template <typename... Args>
  Riemannian::VectorField<Vector, Vector, Args...> gradient() {
    return DeviceGradientField{this, [this](const Vector &x) {
                                 Vector grad(ctx_, 6 * N_);
                                 check(mi_pgo_gradient(prob_, x.handle(), grad.handle()));
                                 return grad;
                               }};
  }
  // 3x3 block-Jacobi over the 2N diagonal blocks; its inverse blocks are refreshed by every quadratic_model() call (TNT
  // calls the model before the preconditioner)
  template <typename... Args>
  Riemannian::LinearOperator<Vector, Vector, Args...> preconditioner() {
    if (!bj_) {
      // bind the (problem-owned) handle now
      Vector tmpx(ctx_, 12 * N_), tmpg(ctx_, 6 * N_);
      check(mi_vec_fill(tmpx.handle(), 0.0));
      mi_op *op = nullptr;
      check(mi_pgo_model(prob_, tmpx.handle(), tmpg.handle(), &op, &bj_));
    }
    return DevicePreconditioner{bj_, this};
  }

  // TNT from x0 with the tagged callables and the block-Jacobi preconditioner
  PoseGraphResult refine(const Vector &x0, const Riemannian::TNTParams<double> &params = Riemannian::TNTParams<double>()) {
    std::optional<Riemannian::LinearOperator<Vector, Vector>> precon = preconditioner();
    const auto r = Riemannian::TNT<Vector, Vector, double>(objective(), quadratic_model(), metric(), retraction(), x0, precon, params);
    PoseGraphResult out;
    out.x = r.x;
    out.f = r.f;
    out.gradient_norm = r.gradfx_norm;
    out.outer_iterations = r.inner_iterations.size();
    for (size_t k : r.inner_iterations) out.inner_iterations += k;
    out.status = r.status;
    return out;
  }

 private:
  Vector retract(const Vector &x, const Vector &eta) const {
    Vector y = Vector::like(x);
    check(mi_pgo_retract(prob_, x.handle(), eta.handle(), y.handle()));
    return y;
  }
  Context ctx_;
  size_t N_, E_;
  mi_pgo *prob_ = nullptr;
  mi_precon *bj_ = nullptr;
};

}  // namespace MI355
}  // namespace Optimization
