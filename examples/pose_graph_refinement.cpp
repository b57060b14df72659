// examples/pose_graph_refinement.cpp -- the maximum-likelihood poses of a noisy synthetic pose graph, end to end on the device:
//   rotations     RotationAveraging::spectral_initialization;
//   translations  TranslationRecovery::solve at those rotations (the chordal initial guess (R, t));
//   refinement    PoseGraph::refine: Riemannian::TNT on SE(3)^N over rotations and positions together,
//                     f(R, t) = 1/2 sum_e kappa_e |R_j - R_i Rt_e|_F^2 + 1/2 sum_e tau_e |t_j - t_i - R_i tt_e|^2,
//                 inner solves in the fused STPCG, one read-back per trial step.
// The graph is the noisy helix walk of examples/chordal_initialization.cpp.  Printed: f at the chordal start and after the
// refinement, and the pose error in the anchored gauge before and after.
//
//   (built by optimization_amd/build.py: build_harness() into examples/bin/; by hand:)
//   g++ -std=c++17 -O2 -I optimization_amd/include -I include examples/pose_graph_refinement.cpp \
//       -L optimization_amd -lmi355opt -Wl,-rpath,$PWD/optimization_amd -o pose_graph_refinement
//   ./pose_graph_refinement [N]        (poses, default 2000)
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <random>
#include <vector>

#include "Optimization/MI355/PoseGraph.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNT.h"

using namespace Optimization;
using MI355::DeviceVector;
using Mat3 = std::array<double, 9>;  // row-major

static Mat3 mul(const Mat3 &A, const Mat3 &B, bool transpose_A = false) {
  Mat3 C{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) C[3 * i + j] += (transpose_A ? A[3 * k + i] : A[3 * i + k]) * B[3 * k + j];
  return C;
}
static Mat3 expm(double x, double y, double z) {  // Rodrigues
  const double th = std::sqrt(x * x + y * y + z * z);
  const double a = th > 1e-8 ? std::sin(th) / th : 1.0, b = th > 1e-8 ? (1 - std::cos(th)) / (th * th) : 0.5;
  const Mat3 K{0, -z, y, z, 0, -x, -y, x, 0};
  const Mat3 K2 = mul(K, K);
  Mat3 R{1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int c = 0; c < 9; ++c) R[c] += a * K[c] + b * K2[c];
  return R;
}

int main(int argc, char **argv) {
  const size_t N = argc > 1 ? (size_t)std::atol(argv[1]) : 2000;
  if (N < 50) return 2;
  const double sigma_R = 0.01, sigma_t = 0.02;
  const size_t turn = 40;  // poses per turn of the helix: loop closures reach one turn back
  try {
    std::mt19937_64 gen(3);
    std::normal_distribution<double> n01(0.0, 1.0);
    // truth: positions on a helix, orientations a smooth walk
    std::vector<Mat3> R(N);
    std::vector<double> t(3 * N);
    R[0] = Mat3{1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (size_t i = 0; i < N; ++i) {
      const double phi = 2 * M_PI * (double)i / (double)turn;
      t[3 * i] = 5 * std::cos(phi), t[3 * i + 1] = 5 * std::sin(phi), t[3 * i + 2] = 0.5 * (double)i / (double)turn;
      if (i) R[i] = mul(R[i - 1], expm(0.05 * n01(gen), 0.05 * n01(gen), 2 * M_PI / (double)turn + 0.05 * n01(gen)));
    }
    std::vector<int32_t> ei, ej;
    for (size_t i = 0; i + 1 < N; ++i) ei.push_back((int32_t)i), ej.push_back((int32_t)(i + 1));
    for (size_t i = turn; i < N; i += 3) ei.push_back((int32_t)i), ej.push_back((int32_t)(i - turn));
    const size_t E = ei.size();
    std::vector<double> Rt(9 * E), tt(3 * E), kappa(E, 1 / (sigma_R * sigma_R)), tau(E, 1 / (sigma_t * sigma_t));
    for (size_t e = 0; e < E; ++e) {
      const size_t i = (size_t)ei[e], j = (size_t)ej[e];
      const Mat3 M = mul(mul(R[i], R[j], true), expm(sigma_R * n01(gen), sigma_R * n01(gen), sigma_R * n01(gen)));
      for (int c = 0; c < 9; ++c) Rt[9 * e + c] = M[c];
      for (int a = 0; a < 3; ++a) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += R[i][3 * k + a] * (t[3 * j + k] - t[3 * i + k]);
        tt[3 * e + a] = s + sigma_t * n01(gen);
      }
    }
    MI355::Context ctx(0);
    // the chordal initial guess: rotations, then positions for those rotations
    MI355::RotationAveraging rot(ctx, N, E, ei.data(), ej.data(), Rt.data(), kappa.data());
    const MI355::SpectralResult s = rot.spectral_initialization();
    std::printf("spectral initialisation: %zu LOBPCG iterations (%s), f_rot(R0) = %.6e\n", s.iterations,
                s.converged ? "converged" : "NOT converged", s.f);
    MI355::TranslationRecovery rec(ctx, N, E, ei.data(), ej.data(), tt.data(), tau.data(), 0);
    const MI355::TranslationResult tr = rec.solve(s.R);
    std::printf("translations: %zu PCG iterations (exit %d), f_tau = %.6e\n", tr.iterations, tr.exit, tr.objective);
    // joint refinement
    MI355::PoseGraph pg(ctx, N, E, ei.data(), ej.data(), Rt.data(), tt.data(), kappa.data(), tau.data());
    const DeviceVector x0 = pg.pack(s.R, tr.t);
    const double f0 = pg.objective()(x0);
    Riemannian::TNTParams<double> params;
    params.gradient_tolerance = 1e-6 / (sigma_R * sigma_R);
    params.preconditioned_gradient_tolerance = 0;
    params.relative_decrease_tolerance = 0;
    params.stepsize_tolerance = 0;
    const MI355::PoseGraphResult r = pg.refine(x0, params);
    std::printf("refinement: f = %.6e at the chordal start -> %.6e after %zu outer / %zu inner iterations, |grad| = %.1e\n", f0, r.f,
                r.outer_iterations, r.inner_iterations, r.gradient_norm);
    // the pose error in the anchored gauge: G = Rhat_0 R_0', Rhat_i ~ G R_i, that_i - that_0 ~ G (t_i - t_0)
    auto pose_error = [&](const std::vector<double> &x, double &er, double &et) {
      Mat3 R0h, R0t{};
      for (int c = 0; c < 9; ++c) R0h[c] = x[c];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R0t[3 * a + b] = R[0][3 * b + a];
      const Mat3 G = mul(R0h, R0t);
      er = et = 0;
      for (size_t i = 0; i < N; ++i) {
        const Mat3 GR = mul(G, R[i]);
        for (int c = 0; c < 9; ++c) er += (x[9 * i + c] - GR[c]) * (x[9 * i + c] - GR[c]);
        for (int a = 0; a < 3; ++a) {
          double s2 = 0;
          for (int k = 0; k < 3; ++k) s2 += G[3 * a + k] * (t[3 * i + k] - t[k]);
          const double d = x[9 * N + 3 * i + a] - x[9 * N + a] - s2;
          et += d * d;
        }
      }
      er = std::sqrt(er / (double)N), et = std::sqrt(et / (double)N);
    };
    double er0, et0, er1, et1;
    pose_error(x0.to_host(), er0, et0);
    pose_error(r.x.to_host(), er1, et1);
    std::printf("pose error in the anchored gauge (rms): rotations %.3e -> %.3e, positions %.3e -> %.3e\n", er0, er1, et0, et1);
    const bool ok = s.converged && r.f <= f0 && r.status == Riemannian::TNTStatus::Gradient;
    std::printf("%s\n", ok ? "refined" : "NOT refined");
    return ok ? 0 : 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 2;
  }
}
