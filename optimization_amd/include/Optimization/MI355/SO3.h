// Optimization/MI355/SO3.h -- ready-made device callables for chordal rotation averaging on SO(3)^N
//     f(R) = 1/2 sum_e w_e | R_j - R_i Rt_e |_F^2
// in the shape the reference's templates expect (Objective, QuadraticModel, RiemannianMetric,
// Retraction, and a LinearOperator preconditioner; Optimization/Riemannian/Concepts.h).  Variable =
// N row-major 3x3 blocks (9N doubles), Tangent = so(3)^N coordinates (3N doubles), metric =
// coordinate dot product, retraction R_i exp(hat(xi_i)), preconditioner = 3x3 block-Jacobi built from
// the Hessian's diagonal blocks.  Kernels: optimization_amd/csrc/so3.hip.
// The same problem as a nonlinear least-squares one, f = 1/2 |F(R)|^2 with F_e = sqrt(w_e) (R_j - R_i Rt_e) in R^{9E}:
// residual(), jacobian(), residual_inner_product() and gauss_newton_preconditioner() are the arguments of
// Riemannian::TNLS (with metric() and retraction() from above); every inner solve then runs in the fused mi_lsqr.
#pragma once

#include <cstdint>

#include "Optimization/LinearAlgebra/Concepts.h"
#include "Optimization/MI355/Device.h"
#include "Optimization/Riemannian/Concepts.h"

namespace Optimization {
namespace MI355 {

class RotationAveraging {
 public:
  using Vector = DeviceVector;

  RotationAveraging(const Context &ctx, size_t N, size_t n_edges, const int32_t *ei, const int32_t *ej,
                    const double *Rt, const double *w)
      : ctx_(ctx), N_(N), E_(n_edges) {
    check(mi_so3n_create(ctx_.get(), N, n_edges, ei, ej, Rt, w, &prob_));
  }
  RotationAveraging(const RotationAveraging &) = delete;
  RotationAveraging &operator=(const RotationAveraging &) = delete;
  ~RotationAveraging() {
    if (prob_) mi_so3n_destroy(prob_);
  }

  size_t rotations() const { return N_; }

  // (every accessor: `Args...` is the extra-argument pack of the caller's signatures -- prob.objective<Cache>() --
  // empty by default.  The tagged objects ignore the pack; a lambda wrapped around them would lose the tag.)
  template <typename... Args>
  Objective<Vector, double, Args...> objective() {
    return DeviceObjective{this, [this](const Vector &R) {
                             double f = 0;
                             check(mi_so3n_objective(prob_, R.handle(), &f));
                             return f;
                           }};
  }
  // gradient in so(3)^N coordinates + the 3x3-block sparse Hessian assembled at R; also refreshes the
  // block-Jacobi preconditioner returned by preconditioner()
  template <typename... Args>
  Riemannian::QuadraticModel<Vector, Vector, Args...> quadratic_model() {
    return [this](const Vector &R, Vector &grad, Riemannian::LinearOperator<Vector, Vector, Args...> &Hess, Args &...) {
      if (grad.empty() || grad.size() != 3 * N_) grad = Vector(ctx_, 3 * N_);
      mi_op *op = nullptr;
      check(mi_so3n_model(prob_, R.handle(), grad.handle(), &op, &bj_));
      Hess = DeviceHessian{op, this};
    };
  }
  template <typename... Args>
  Riemannian::RiemannianMetric<Vector, Vector, double, Args...> metric() {
    return FrobeniusMetric{};
  }
  // R_i exp(hat(xi_i)) -- tagged: TNT evaluates a whole trial step (retraction, f at the trial point, the
  // predicted-decrease terms, the model and both gradient norms at the trial point) through mi_so3n_trial, one read-back;
  // GradientDescent evaluates a whole Armijo trial (h = -t g, retraction, f and the gradient norm at the trial point)
  // through mi_so3n_armijo_trial, one read-back
  template <typename... Args>
  Riemannian::Retraction<Vector, Vector, Args...> retraction() {
    DeviceTrialRetraction r;
    r.owner = this;
    r.retract = [this](const Vector &R, const Vector &xi) {
      Vector Y = Vector::like(R);
      check(mi_so3n_retract(prob_, R.handle(), xi.handle(), Y.handle()));
      return Y;
    };
    r.trial = [this](const Vector &R, const Vector &h, const Vector &g, bool with_precon) {
      DeviceTrialRetraction::Trial t;
      t.x_trial = Vector::like(R);
      double out[6];
      check(mi_so3n_trial(prob_, R.handle(), h.handle(), g.handle(), with_precon ? 1 : 0, t.x_trial.handle(), out));
      t.f_trial = out[0];
      t.hh = out[1];
      t.gh = out[2];
      t.hHh = out[3];
      t.grad_trial_sqnorm = out[4];
      t.precon_grad_trial_sqnorm = out[5];
      return t;
    };
    r.armijo = [this](const Vector &R, const Vector &g, double t) {
      DeviceTrialRetraction::ArmijoTrial a;
      a.h = Vector::like(g);
      a.x_trial = Vector::like(R);
      double out[2];
      check(mi_so3n_armijo_trial(prob_, R.handle(), g.handle(), t, a.h.handle(), a.x_trial.handle(), out));
      a.f_trial = out[0];
      a.grad_trial_sqnorm = out[1];
      return a;
    };
    return r;
  }
  // grad f(R) in so(3)^N coordinates as a VectorField (GradientDescent's interface): the gradient-only assembly pass --
  // no Hessian blocks, nothing bound; after a fused trial at R it is already there
  template <typename... Args>
  Riemannian::VectorField<Vector, Vector, Args...> gradient() {
    return DeviceGradientField{this, [this](const Vector &R) {
                                 Vector grad(ctx_, 3 * N_);
                                 check(mi_so3n_gradient(prob_, R.handle(), grad.handle()));
                                 return grad;
                               }};
  }
  // the same without the tag (one call per statement of the reference's loop)
  Riemannian::Retraction<Vector, Vector> plain_retraction() {
    return [this](const Vector &R, const Vector &xi) {
      Vector Y = Vector::like(R);
      check(mi_so3n_retract(prob_, R.handle(), xi.handle(), Y.handle()));
      return Y;
    };
  }
  // --- Riemannian::TNLS ------------------------------------------------------------------------------------------
  //   Riemannian::TNLS<Vector, Vector, Vector>(prob.residual(), prob.jacobian(), prob.metric(),
  //                                            prob.residual_inner_product(), prob.retraction(), R0, precon, params)
  // F(R): 9 doubles per edge, the caller's edge order (mi_so3n_residual)
  size_t edges() const { return E_; }
  template <typename... Args>
  Riemannian::Mapping<Vector, Vector, Args...> residual() {
    return [this](const Vector &R, Args &...) {
      Vector F(ctx_, 9 * E_);
      check(mi_so3n_residual(prob_, R.handle(), F.handle(), nullptr));
      return F;
    };
  }
  // (dF_R, dF_R^*) as tagged device operators bound to R (mi_so3n_jacobian): typed without the pack, as TNLS takes it.
  // The handles are the problem's and are rebound by every call: the pair of the latest linearisation is the valid one.
  Riemannian::JacobianPairFunction<Vector, Vector, Vector> jacobian() {
    return [this](const Vector &R) {
      mi_op *a = nullptr, *at = nullptr;
      check(mi_so3n_jacobian(prob_, R.handle(), &a, &at));
      return std::make_pair(Riemannian::Jacobian<Vector, Vector, Vector>(DeviceHessian{a, this}),
                            Riemannian::JacobianAdjoint<Vector, Vector, Vector>(DeviceHessian{at, this}));
    };
  }
  template <typename... Args>
  LinearAlgebra::InnerProduct<Vector, double, Args...> residual_inner_product() {
    return FrobeniusInnerProduct{};
  }
  // the right preconditioner pair (M, M') of TNLS, M = M' = diag(1 / sqrt(2 degw_i)): the diagonal blocks of dF* dF are
  // 2 degw_i I, so this is the block-Jacobi scaling of the Gauss-Newton system (mi_so3n_gn_scaling)
  template <typename... Args>
  std::pair<Riemannian::LinearOperator<Vector, Vector, Args...>, Riemannian::LinearOperator<Vector, Vector, Args...>>
  gauss_newton_preconditioner() {
    mi_op *m = nullptr;
    check(mi_so3n_gn_scaling(prob_, &m));
    return std::make_pair(Riemannian::LinearOperator<Vector, Vector, Args...>(DeviceHessian{m, this}),
                          Riemannian::LinearOperator<Vector, Vector, Args...>(DeviceHessian{m, this}));
  }
  // 3x3 block-Jacobi; valid after the first quadratic_model() call (TNT calls QM before precon)
  template <typename... Args>
  Riemannian::LinearOperator<Vector, Vector, Args...> preconditioner() {
    if (!bj_) {
      // bind the (problem-owned) handle now; its inverse blocks are refreshed by every model call
      Vector tmpR(ctx_, 9 * N_), tmpg(ctx_, 3 * N_);
      check(mi_vec_fill(tmpR.handle(), 0.0));
      mi_op *op = nullptr;
      check(mi_so3n_model(prob_, tmpR.handle(), tmpg.handle(), &op, &bj_));
    }
    return DevicePreconditioner{bj_, this};
  }

 private:
  Context ctx_;
  size_t N_, E_;
  mi_so3n *prob_ = nullptr;
  mi_precon *bj_ = nullptr;
};

}  // namespace MI355
}  // namespace Optimization
