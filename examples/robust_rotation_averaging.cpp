// robust_rotation_averaging.cpp -- rotation averaging with outliers: graduated non-convexity (GNC) around Riemannian::TNT.
// A ring of N rotations with chords, measurements R_i' R_j with 0.02 rad of noise, every tenth one replaced by a random
// rotation.  One plain (L2) solve, then rounds of
//     prob.reweight(R, {GemanMcClure, c sqrt(mu)})   -- w_e = (mu c^2 / (r_e^2 + mu c^2))^2 on the device, no rebuild
//     R = TNT(...)
// with mu halved each round, and the global-optimality certificate of the final weighted problem.
#include <cmath>
#include <cstdio>
#include <optional>
#include <random>
#include <vector>

#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNT.h"

using namespace Optimization;
namespace RM = Optimization::Riemannian;
using MI355::DeviceVector;

static void mul(const double *A, const double *B, double *C, bool At = false) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (At ? A[3 * k + i] : A[3 * i + k]) * B[3 * k + j];
      C[3 * i + j] = s;
    }
}
static void expm(const double *x, double *R) {  // Rodrigues
  const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], th = std::sqrt(th2);
  const double a = th < 1e-8 ? 1 : std::sin(th) / th, b = th < 1e-8 ? .5 : (1 - std::cos(th)) / th2;
  const double K[9] = {0, -x[2], x[1], x[2], 0, -x[0], -x[1], x[0], 0};
  double K2[9];
  mul(K, K, K2);
  for (int c = 0; c < 9; ++c) R[c] = (c % 4 == 0 ? 1 : 0) + a * K[c] + b * K2[c];
}

int main() {
  const size_t N = 2000;
  std::mt19937_64 gen(7);
  std::normal_distribution<double> nrm;
  auto random_rotation = [&](double scale, double *R) {
    const double x[3] = {scale * nrm(gen), scale * nrm(gen), scale * nrm(gen)};
    expm(x, R);
  };
  std::vector<double> truth(9 * N), R0(9 * N);
  for (size_t i = 0; i < N; ++i) {
    random_rotation(1.5, &truth[9 * i]);
    double P[9];
    random_rotation(0.3, P);
    mul(&truth[9 * i], P, &R0[9 * i]);
  }
  std::vector<int32_t> ei, ej;
  for (size_t i = 0; i < N; ++i) {
    ei.push_back((int32_t)i); ej.push_back((int32_t)((i + 1) % N));
    ei.push_back((int32_t)i); ej.push_back((int32_t)((i * 7 + 13) % N == i ? (i + 2) % N : (i * 7 + 13) % N));
  }
  const size_t E = ei.size();
  std::vector<double> Rt(9 * E), w(E, 1.0);
  size_t planted = 0;
  for (size_t e = 0; e < E; ++e) {
    if (e % 10 == 3) {
      random_rotation(1.5, &Rt[9 * e]);
      ++planted;
      continue;
    }
    double D[9], Nz[9];
    mul(&truth[9 * ei[e]], &truth[9 * ej[e]], D, true);
    random_rotation(0.02, Nz);
    mul(D, Nz, &Rt[9 * e]);
  }
  auto mean_error = [&](const std::vector<double> &R) {  // mean angle of (G R_i)' T_i, G = T_0 R_0' (gauge fixed at node 0)
    double G[9], R0t[9];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) R0t[3 * a + b] = R[3 * b + a];
    mul(&truth[0], R0t, G);
    double s = 0;
    for (size_t i = 0; i < N; ++i) {
      double GR[9], D[9];
      mul(G, &R[9 * i], GR);
      mul(GR, &truth[9 * i], D, true);
      s += std::acos(std::fmax(-1.0, std::fmin(1.0, (D[0] + D[4] + D[8] - 1) / 2)));
    }
    return s / (double)N;
  };

  MI355::Context ctx(0);
  MI355::RotationAveraging prob(ctx, N, E, ei.data(), ej.data(), Rt.data(), w.data());
  RM::TNTParams<double> tp;
  tp.max_iterations = 100;
  tp.gradient_tolerance = 1e-8;
  auto solve = [&](const DeviceVector &start) {
    std::optional<RM::LinearOperator<DeviceVector, DeviceVector>> pc = prob.preconditioner();
    return RM::TNT<DeviceVector, DeviceVector>(prob.objective(), prob.quadratic_model(), prob.metric(), prob.retraction(),
                                               start, pc, tp)
        .x;
  };
  DeviceVector R = solve(DeviceVector(ctx, R0.data(), 9 * N));
  std::printf("%zu rotations, %zu measurements, %zu of them planted outliers\n", N, E, planted);
  std::printf("L2 solve:            mean angular error %.4f rad\n", mean_error(R.to_host()));
  const double c = 0.15;
  double mu = 64;
  for (int round = 0; round < 6; ++round, mu *= .5) {
    const MI355::ReweightInfo info = prob.reweight(R, {MI355::RobustKernel::GemanMcClure, c * std::sqrt(mu)});
    R = solve(R);
    std::printf("GNC round %d (mu %5.1f): robust cost %.4f, %zu edges with weight factor < 1/2, mean angular error %.4f rad\n",
                round, mu, info.robust_cost, info.outliers, mean_error(R.to_host()));
  }
  const MI355::CertifyResult cert = prob.certify(R);
  std::printf("final weighted problem: lambda_min(S) = %.3e, %s\n", cert.lambda_min,
              cert.certified ? "certified globally optimal" : "not certified");
  return 0;
}
