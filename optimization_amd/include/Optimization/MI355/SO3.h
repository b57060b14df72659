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
// A start point: spectral_initialization() rounds the three lowest eigenvectors of the connection Laplacian
// (laplacian_operator(), LOBPCG) to SO(3)^N; project() takes a point with an orthogonality defect back onto it.
// Global optimality: certificate_operator(R) is the certificate matrix S(R) of mi_so3n_certificate as a
// SymmetricLinearOperator on device panels, certify(R) its smallest eigenvalue through LinearAlgebra::LOBPCG and the
// verdict that follows from it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <optional>
#include <vector>

#include "Optimization/LinearAlgebra/Concepts.h"
#include "Optimization/LinearAlgebra/LOBPCG.h"
#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/Matrix.h"
#include "Optimization/Riemannian/Concepts.h"

namespace Optimization {
namespace MI355 {

// The certificate matrix S(R) (mi355opt.h: mi_so3n_certificate) as a callable on column-major 3N x k device panels --
// tagged: what RotationAveraging::certificate_operator returns inside a SymmetricLinearOperator<DeviceMatrix>, to be found
// again with std::function::target.  The handle is the problem's and is rebound by the next certificate_operator() /
// certify() call: the operator of the latest call is the valid one.
struct CertificateOperator {
  mi_so3n_cert *cert = nullptr;
  const void *owner = nullptr;
  size_t N = 0;
  double f = 0;             // f(R), the bits of mi_so3n_objective
  double stationarity = 0;  // |skew Q|_F = |S Y|_F
  double trace_C = 0;       // sum_i tr C_i
  DeviceMatrix operator()(const DeviceMatrix &X) const {
    DeviceMatrix Z(X.context(), X.rows(), X.cols());
    check(mi_so3n_cert_apply(cert, (int)X.cols(), X.handle(), Z.handle()));
    return Z;
  }
  // S [block 0 | block 1 | ...] of a panel held as column blocks: nothing is copied together
  DeviceMatrix operator()(const PanelBlocks &X) const {
    DeviceMatrix Z(X.context(), X.rows(), X.cols());
    const mi_panel_blocks b = X.raw();
    check(mi_so3n_cert_apply_blocks(cert, &b, Z.handle()));
    return Z;
  }
};

struct CertifyParams {
  size_t nx = 6;                 // block size of the eigensolver (at most N): wider than the eigenvalue cluster at 0
  double tau = 1e-8;             // LOBPCG's relative residual tolerance
  size_t max_iterations = 1000;
  double eta = -1;               // certified <=> converged and lambda_min_safe >= -eta; negative: the default (see certify)
  std::optional<LinearAlgebra::SymmetricLinearOperator<DeviceMatrix>> preconditioner;  // LOBPCG's T
};
struct CertifyResult {
  double lambda_min = 0;       // theta_0, the smallest Ritz value
  double lambda_min_safe = 0;  // theta_0 - |r_0| / |x_0|: no eigenvalue-free interval [theta_0 - |r|/|x|, theta_0 + |r|/|x|]
  DeviceMatrix eigenvector;    // 3N x 1 (empty when no solve was needed)
  double f = 0;                // f(R)
  double lower_bound = 0;      // f + 1.5 N min(lambda_min_safe, 0) <= min over O(3)^N of f, PROVIDED theta_0 tracks the smallest
                               // eigenvalue of S (LOBPCG converges to it from a generic start block; it is not proved to)
  double stationarity = 0;     // |skew Q|_F
  double norm_estimate = 0;    // |S| from one Gaussian probe
  double eta = 0;              // the threshold used
  size_t iterations = 0;
  bool converged = false, certified = false;
};

// The connection Laplacian (mi355opt.h: mi_so3n_laplacian) as a callable on column-major 3N x k device panels, tagged as
// CertificateOperator is.  The handle is the problem's, in a slot of its own; its diagonal is that of the latest
// laplacian_operator() / spectral_initialization() call (the weights then in force).
struct LaplacianOperator {
  mi_so3n_cert *lap = nullptr;
  const void *owner = nullptr;
  size_t N = 0;
  DeviceMatrix operator()(const DeviceMatrix &X) const {
    DeviceMatrix Z(X.context(), X.rows(), X.cols());
    check(mi_so3n_cert_apply(lap, (int)X.cols(), X.handle(), Z.handle()));
    return Z;
  }
  DeviceMatrix operator()(const PanelBlocks &X) const {
    DeviceMatrix Z(X.context(), X.rows(), X.cols());
    const mi_panel_blocks b = X.raw();
    check(mi_so3n_cert_apply_blocks(lap, &b, Z.handle()));
    return Z;
  }
};
// Z = D^-1 X, D = degw_i on the rows of node i (mi_so3n_lap_jacobi): LOBPCG's T for the Laplacian
struct LaplacianJacobi {
  mi_so3n *prob = nullptr;
  const void *owner = nullptr;
  DeviceMatrix operator()(const DeviceMatrix &X) const {
    DeviceMatrix Z(X.context(), X.rows(), X.cols());
    check(mi_so3n_lap_jacobi(prob, (int)X.cols(), X.handle(), Z.handle()));
    return Z;
  }
};

struct RoundInfo {
  size_t negative = 0;       // blocks with det < 0 as given
  bool flipped = false;      // the panel was rounded as -V (round only)
  size_t degenerate = 0;     // blocks replaced by the identity
  double min_separation = 0; // round: min (sigma_2 + d sigma_3) / sigma_1 over the other blocks
  double defect = 0;         // project: max |M_i' M_i - I|_F over the other blocks
};
struct SpectralParams {
  size_t nx = 6;             // block size of the eigensolver (at least 3)
  double tau = 1e-6;         // LOBPCG's relative residual tolerance
  size_t max_iterations = 1000;
  bool precondition = true;  // T = the Laplacian's Jacobi scaling
};
struct SpectralResult {
  DeviceVector R;                      // the rounded point, 9N
  DeviceMatrix eigenvectors;           // 3N x 3: what was rounded (empty when no solve was needed)
  double eigenvalues[3] = {0, 0, 0};   // the three lowest Ritz values of the Laplacian
  double f = 0;                        // f(R)
  double lower_bound = 0;              // (N / 2) sum_i (theta_i - |r_i| / |x_i|) <= min f when every measurement is a rotation
                                       // (NaN otherwise), PROVIDED the theta_i track the three smallest eigenvalues (LOBPCG
                                       // converges to them from a generic start block; it is not proved to: see certify)
  size_t iterations = 0;
  bool converged = false, flipped = false;
  size_t degenerate = 0;
  double min_separation = 0;
};

// A robust loss for RotationAveraging::reweight (mi355opt.h: mi_so3n_reweight): the weight function phi(r; c) applied to
// the creation-time weights.  GNC with the Geman-McClure surrogate: {GemanMcClure, c * std::sqrt(mu)}.
struct RobustKernel {
  enum Kind { L2 = MI_ROBUST_L2, Huber = MI_ROBUST_HUBER, Cauchy = MI_ROBUST_CAUCHY, GemanMcClure = MI_ROBUST_GEMAN_MCCLURE } kind = L2;
  double c = 1;
};
struct ReweightInfo {
  double robust_cost = 0;    // sum_e w0_e rho(r_e)
  double weighted_cost = 0;  // sum_e w_e r_e^2 / 2 with the NEW weights: the objective at the same point
  size_t outliers = 0;       // edges with phi < 1/2
};

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
  // --- global optimality ------------------------------------------------------------------------------------------
  // S(R) as LOBPCG's operator A (a CertificateOperator inside: target<CertificateOperator>() has f, the stationarity
  // defect and the panel Y).  Bound to a copy of what depends on R: trial steps, model calls and writes to R leave it alone.
  LinearAlgebra::SymmetricLinearOperator<DeviceMatrix> certificate_operator(const Vector &R) {
    CertificateOperator op;
    op.owner = this;
    op.N = N_;
    double info[3];
    check(mi_so3n_certificate(prob_, R.handle(), &op.cert, info));
    op.f = info[0];
    op.stationarity = info[1];
    op.trace_C = info[2];
    return op;
  }
  // Is the critical point R the global minimiser?  lambda_min(S(R)) by LOBPCG (nev = 1) from a Gaussian start block, drawn
  // like gaussian_probe with the default-seeded engine.  The block is wider than the three eigenvalues S always has at (or
  // near) 0 -- S Y = 0 at a critical point -- so the cluster does not slow the lowest pair down.  Y itself is NOT put into
  // the start block: its columns are eigenvectors with a residual of rounding size (exactly 0 for the axis column of the
  // winding), which the solver's equilibrated Rayleigh-Ritz step cannot take ("B is not positive definite"), and with
  // nev = 1 the solver would stop on one of them after one iteration, before a negative eigenvalue of a large graph has
  // entered the search space.  mi_so3n_cert_null_panel hands Y to clients that deflate it themselves.
  // certified <=> converged and lambda_min_safe >= -eta, by default eta = 2 tau |S|est + stationarity -- what the
  // eigenvalue cannot resolve: the solver's own residual test, and the distance of Y from an exact null vector.
  CertifyResult certify(const Vector &R, const CertifyParams &params = CertifyParams()) {
    const auto A = certificate_operator(R);
    return certify_with(A, *A.target<CertificateOperator>(), params);
  }
  // the same with the operator handed to LOBPCG as given (e.g. `info` wrapped in a plain lambda)
  CertifyResult certify_with(const LinearAlgebra::SymmetricLinearOperator<DeviceMatrix> &A, const CertificateOperator &info,
                             const CertifyParams &params) {
    using Op = LinearAlgebra::SymmetricLinearOperator<DeviceMatrix>;
    CertifyResult out;
    out.f = info.f;
    out.stationarity = info.stationarity;
    if (E_ == 0) {  // S = 0
      out.lower_bound = out.f;
      out.converged = out.certified = true;
      return out;
    }
    const size_t m = 3 * N_, nx = std::max<size_t>(1, std::min(params.nx, N_));
    const DeviceMatrix X0 = gaussian_probe(DeviceMatrix(ctx_, 1, 1), m, nx);
    out.norm_estimate = A(X0).norm() / X0.norm();  // (the estimate LOBPCG forms from its own probe: the same draw)
    out.eta = params.eta >= 0 ? params.eta : 2 * params.tau * out.norm_estimate + out.stationarity;
    size_t iters = 0, nc = 0;
    const size_t nev = 1;
    auto tx = LinearAlgebra::LOBPCG<HostVectorD, DeviceMatrix, double>(A, std::optional<Op>(), params.preconditioner, X0, nev,
                                                                       params.max_iterations, iters, nc, params.tau);
    out.lambda_min = tx.first(0);
    const DeviceMatrix x0col = tx.second.leftCols(1);
    out.eigenvector = x0col;  // (a copy: its storage is its own)
    HostVectorD theta(1, out.lambda_min), r, xn;
    (void)residual_and_norms(A(out.eigenvector), out.eigenvector, out.eigenvector, theta, r, xn);
    out.lambda_min_safe = out.lambda_min - r(0) / xn(0);
    out.lower_bound = out.f + 1.5 * (double)N_ * std::min(out.lambda_min_safe, 0.0);
    out.iterations = iters;
    out.converged = nc == nev;
    out.certified = out.converged && out.lambda_min_safe >= -out.eta;
    return out;
  }
  // --- spectral initialisation -------------------------------------------------------------------------------------
  // A start point without one: the three lowest eigenvectors of the connection Laplacian, each 3 x 3 block rounded to the
  // nearest rotation.  Outside the method and NOT detected: a disconnected graph (more than three eigenvalues at 0: the
  // blocks of different components come out in unrelated gauges) and weights <= 0.
  // The Laplacian with the weights in force as LOBPCG's operator A (a LaplacianOperator inside)
  LinearAlgebra::SymmetricLinearOperator<DeviceMatrix> laplacian_operator() {
    LaplacianOperator op;
    op.owner = this;
    op.N = N_;
    check(mi_so3n_laplacian(prob_, &op.lap));
    return op;
  }
  // its Jacobi scaling as LOBPCG's T (reads the diagonal of the latest laplacian_operator() call)
  LinearAlgebra::SymmetricLinearOperator<DeviceMatrix> laplacian_preconditioner() { return LaplacianJacobi{prob_, this}; }
  // the 3N x 3 panel V block by block to SO(3), after the global sign (mi_so3n_round); info: one read-back, else none
  Vector round(const DeviceMatrix &V, RoundInfo *info = nullptr) {
    Vector R(ctx_, 9 * N_);
    double buf[4];
    check(mi_so3n_round(prob_, V.handle(), R.handle(), info ? buf : nullptr));
    if (info) {
      info->negative = (size_t)buf[0];
      info->flipped = buf[1] != 0;
      info->degenerate = (size_t)buf[2];
      info->min_separation = buf[3];
    }
    return R;
  }
  // a 9N point with an orthogonality defect back onto SO(3)^N (mi_so3n_project)
  Vector project(const Vector &M, RoundInfo *info = nullptr) {
    Vector R(ctx_, 9 * N_);
    double buf[3];
    check(mi_so3n_project(prob_, M.handle(), R.handle(), info ? buf : nullptr));
    if (info) {
      info->defect = buf[0];
      info->degenerate = (size_t)buf[1];
      info->negative = (size_t)buf[2];
    }
    return R;
  }
  // LOBPCG (nev = 3) on the Laplacian from the default-seeded gaussian_probe block, then round.  A problem of at most
  // kSpectralDenseRows = 96 rows (N <= 32: one panel of the widest product) is solved densely on the host instead
  // (iterations = 0).  E == 0 returns identities without a solve.
  static constexpr size_t kSpectralDenseRows = 96;
  SpectralResult spectral_initialization(const SpectralParams &params = SpectralParams()) {
    using Op = LinearAlgebra::SymmetricLinearOperator<DeviceMatrix>;
    SpectralResult out;
    const size_t m = 3 * N_, nev = 3;
    if (E_ == 0) {
      std::vector<double> eye(9 * N_, 0.0);
      for (size_t i = 0; i < N_; ++i) eye[9 * i] = eye[9 * i + 4] = eye[9 * i + 8] = 1.0;
      out.R = Vector(ctx_, eye);
      out.converged = true;
      out.min_separation = 2;
      return out;
    }
    const Op A = laplacian_operator();
    const size_t nx = std::max(nev, params.nx);
    HostVectorD theta;
    DeviceMatrix V;
    if (m <= kSpectralDenseRows) {
      // the Laplacian read off the device operator (Lap I) and solved on the host: exact, and LOBPCG's basis of 3 nx
      // columns is not asked to stay independent in a space that is hardly larger
      std::vector<double> eye(m * m, 0.0);
      for (size_t i = 0; i < m; ++i) eye[i + i * m] = 1.0;
      const std::vector<double> lap = A(DeviceMatrix(ctx_, m, m, eye.data())).to_host();
      HostMatrix Lh(m, m), Ih(m, m);
      std::copy(lap.begin(), lap.end(), Lh.data());
      std::copy(eye.begin(), eye.end(), Ih.data());
      auto tc = rayleigh_ritz(Lh, Ih);
      theta = tc.first.head(nev);
      V = DeviceMatrix(ctx_, m, nev, tc.second.data());
      out.converged = true;
    } else {
      const DeviceMatrix X0 = gaussian_probe(DeviceMatrix(ctx_, 1, 1), m, nx);
      const std::optional<Op> T = params.precondition ? std::optional<Op>(laplacian_preconditioner()) : std::optional<Op>();
      size_t iters = 0, nc = 0;
      auto tx = LinearAlgebra::LOBPCG<HostVectorD, DeviceMatrix, double>(A, std::optional<Op>(), T, X0, nev,
                                                                         params.max_iterations, iters, nc, params.tau);
      theta = tx.first;
      V = std::move(tx.second);
      out.iterations = iters;
      out.converged = nc == nev;
    }
    HostVectorD r, xn;
    (void)residual_and_norms(A(V), V, V, theta, r, xn);
    size_t forms[6];
    check(mi_debug_so3n_info(prob_, forms));
    double safe = 0;
    for (size_t i = 0; i < nev; ++i) {
      out.eigenvalues[i] = theta(i);
      safe += theta(i) - r(i) / xn(i);
    }
    out.lower_bound = forms[0] ? .5 * (double)N_ * safe : std::nan("");
    RoundInfo info;
    out.R = round(V, &info);
    out.flipped = info.flipped;
    out.degenerate = info.degenerate;
    out.min_separation = info.min_separation;
    check(mi_so3n_objective(prob_, out.R.handle(), &out.f));
    out.eigenvectors = std::move(V);
    return out;
  }
  // --- robust loss -------------------------------------------------------------------------------------------------
  // w_e <- w0_e phi(|R_j - R_i Rt_e|_F) on the device (mi_so3n_reweight; one read-back for the info).  The problem drops the
  // model bound to any point, the speculative model and gradient of its trial chain and with them every point key: the
  // class keeps none of its own (objective(), quadratic_model(), retraction() ... go to the problem handle each time), so a
  // TNT / GradientDescent / TNLS call after this assembles at its start point with the new weights.  Operators handed out
  // BEFORE (jacobian(), certificate_operator()) are to be requested again; gauss_newton_preconditioner() and
  // preconditioner() stay valid.
  ReweightInfo reweight(const Vector &R, const RobustKernel &k) {
    double info[3];
    check(mi_so3n_reweight(prob_, R.handle(), (int)k.kind, k.c, info));
    ReweightInfo out;
    out.robust_cost = info[0];
    out.weighted_cost = info[1];
    out.outliers = (size_t)info[2];
    return out;
  }
  // back to the creation-time weights (no read-back)
  void reset_weights() { check(mi_so3n_reweight(prob_, nullptr, MI_ROBUST_L2, 1.0, nullptr)); }
  // the weights in force, the caller's edge order
  std::vector<double> weights() const {
    std::vector<double> w(E_);
    check(mi_so3n_weights(prob_, w.data()));
    return w;
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
