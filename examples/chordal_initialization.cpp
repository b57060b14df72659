// examples/chordal_initialization.cpp -- the poses of a noisy synthetic pose graph, rotations first, then translations:
//   rotations     RotationAveraging::spectral_initialization, then Riemannian::TNT from that point;
//   translations  TranslationRecovery::solve at the rotations TNT reached: the linear least-squares problem
//                 min_t 1/2 sum_e tau_e |t_j - t_i - R_i tt_e|^2 in the gauge t_0 = 0, one fused PCG solve on the device.
// The graph is a noisy walk along a helix (odometry edges i -> i + 1) with loop closures to the turn below; measurements
// Rt_e = R_i' R_j exp(sigma_R n), tt_e = R_i'(t_j - t_i) + sigma_t n.  Printed: the pose error in the anchored gauge (the
// estimate aligned with the truth at pose 0), which should be a small multiple of the noise level.
//
//   (built by optimization_amd/build.py: build_harness() into examples/bin/; by hand:)
//   g++ -std=c++17 -O2 -I optimization_amd/include -I include examples/chordal_initialization.cpp \
//       -L optimization_amd -lmi355opt -Wl,-rpath,$PWD/optimization_amd -o chordal_initialization
//   ./chordal_initialization [N]        (poses, default 2000)
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
    // rotations
    MI355::RotationAveraging rot(ctx, N, E, ei.data(), ej.data(), Rt.data(), kappa.data());
    const MI355::SpectralResult s = rot.spectral_initialization();
    std::printf("spectral initialisation: %zu LOBPCG iterations (%s), f(R0) = %.6e\n", s.iterations,
                s.converged ? "converged" : "NOT converged", s.f);
    Riemannian::TNTParams<double> params;
    params.gradient_tolerance = 1e-6 / (sigma_R * sigma_R);
    params.relative_decrease_tolerance = 0;
    params.stepsize_tolerance = 0;
    std::optional<Riemannian::LinearOperator<DeviceVector, DeviceVector>> pc = rot.preconditioner();
    auto res = Riemannian::TNT<DeviceVector, DeviceVector>(rot.objective(), rot.quadratic_model(), rot.metric(),
                                                           rot.retraction(), s.R, pc, params);
    std::printf("TNT: %zu outer iterations, f = %.6e, |grad| = %.1e\n", res.inner_iterations.size(), res.f, res.gradfx_norm);
    // translations
    MI355::TranslationRecovery rec(ctx, N, E, ei.data(), ej.data(), tt.data(), tau.data(), 0);
    const MI355::TranslationResult tr = rec.solve(res.x);
    std::printf("translations: %zu PCG iterations (exit %d), f_tau = %.6e, |L t - b| / |b| = %.1e, max |r_e| = %.3e\n",
                tr.iterations, tr.exit, tr.objective, tr.relative_residual, tr.max_residual);
    // the pose error in the anchored gauge: G = Rhat_0 R_0', Rhat_i ~ G R_i, that_i ~ G (t_i - t_0)
    const std::vector<double> Rh = res.x.to_host(), th = tr.t.to_host();
    Mat3 R0h;
    for (int c = 0; c < 9; ++c) R0h[c] = Rh[c];
    Mat3 R0t{};  // R_0'
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) R0t[3 * a + b] = R[0][3 * b + a];
    const Mat3 G = mul(R0h, R0t);
    double er = 0, et = 0, extent = 0;
    for (size_t i = 0; i < N; ++i) {
      const Mat3 GR = mul(G, R[i]);
      for (int c = 0; c < 9; ++c) er += (Rh[9 * i + c] - GR[c]) * (Rh[9 * i + c] - GR[c]);
      double d2 = 0;
      for (int a = 0; a < 3; ++a) {
        double s2 = 0;
        for (int k = 0; k < 3; ++k) s2 += G[3 * a + k] * (t[3 * i + k] - t[k]);
        et += (th[3 * i + a] - s2) * (th[3 * i + a] - s2);
        d2 += (t[3 * i + a] - t[a]) * (t[3 * i + a] - t[a]);
      }
      extent = std::max(extent, std::sqrt(d2));
    }
    er = std::sqrt(er / (double)N), et = std::sqrt(et / (double)N);
    std::printf("pose error in the anchored gauge: rotations rms |Rhat_i - G R_i|_F = %.3e (sigma_R = %.0e), "
                "positions rms = %.3e (sigma_t = %.0e, extent %.1f)\n", er, sigma_R, et, sigma_t, extent);
    const bool ok = s.converged && tr.exit == MI_STPCG_EXIT_RESIDUAL && er <= 10 * sigma_R && et <= 10 * (sigma_t + sigma_R * extent);
    std::printf("%s\n", ok ? "consistent with the noise level" : "NOT consistent with the noise level");
    return ok ? 0 : 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 2;
  }
}
