// Optimization/MI355/PoseGraph.h -- the translation half of a pose graph on the device.
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
#include <utility>
#include <vector>

#include "Optimization/LinearAlgebra/Concepts.h"
#include "Optimization/LinearAlgebra/IterativeSolvers.h"
#include "Optimization/MI355/Device.h"

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

}  // namespace MI355
}  // namespace Optimization
