// examples/certify_rotation_averaging.cpp -- is the point a rotation-averaging solver returned the GLOBAL minimiser?
// Riemannian::TNT on MI355::RotationAveraging, then RotationAveraging::certify: the smallest eigenvalue of the
// certificate matrix S(R) = Lap - BlockDiag(sym(R_i' (L R)_i)) by the device LOBPCG.  Two cases:
//   a ring with random chords and noisy measurements, solved from the ground truth: certified;
//   a cycle with identity measurements at the winding R_i = rot_z(2 pi i / N), a critical point that TNT does not leave
//   (its gradient is zero): lambda_min = 2 cos(2 pi / N) - 2 < 0, not certified.
//
//   (built by optimization_amd/build.py: build_harness() into examples/bin/; by hand:)
//   g++ -std=c++17 -O2 -I optimization_amd/include -I include examples/certify_rotation_averaging.cpp \
//       -L optimization_amd -lmi355opt -Wl,-rpath,$PWD/optimization_amd -o certify_rotation_averaging
//   ./certify_rotation_averaging [N]        (rotations, default 200)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <random>
#include <vector>

#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNT.h"

using namespace Optimization;
using MI355::DeviceVector;

namespace {

void rodrigues(const double v[3], double *R) {  // exp(hat(v)), row-major
  const double t = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double a = t < 1e-12 ? 1.0 : std::sin(t) / t, b = t < 1e-12 ? 0.5 : (1 - std::cos(t)) / (t * t);
  const double K[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double k2 = 0;
      for (int l = 0; l < 3; ++l) k2 += K[i * 3 + l] * K[l * 3 + j];
      R[i * 3 + j] = (i == j) + a * K[i * 3 + j] + b * k2;
    }
}
void mul(const double *A, bool At, const double *B, double *C) {  // C = A B or A' B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int l = 0; l < 3; ++l) s += (At ? A[l * 3 + i] : A[i * 3 + l]) * B[l * 3 + j];
      C[i * 3 + j] = s;
    }
}

bool report(const char *what, MI355::RotationAveraging &prob, const DeviceVector &R, bool expect) {
  const MI355::CertifyResult c = prob.certify(R);
  std::printf("%s: f = %.6e, |skew Q| = %.1e, lambda_min = %.6e (safe %.6e, eta %.1e) after %zu LOBPCG iterations\n", what,
              c.f, c.stationarity, c.lambda_min, c.lambda_min_safe, c.eta, c.iterations);
  std::printf("    lower bound on the optimum %.6e  =>  %s\n", c.lower_bound,
              c.certified ? "CERTIFIED global minimiser" : "not certified");
  return c.converged && c.certified == expect;
}

}  // namespace

int main(int argc, char **argv) {
  const size_t N = argc > 1 ? (size_t)std::atol(argv[1]) : 200;
  if (N < 5) return 2;
  try {
    MI355::Context ctx(0);
    bool ok = true;
    {  // (a) a ring with N / 2 chords, rotation noise 0.1, solved by TNT from the ground truth
      std::mt19937_64 rng(11);
      std::normal_distribution<double> nrm;
      std::uniform_real_distribution<double> uw(0.5, 2.0);
      std::vector<double> Rgt(9 * N), Rt, w;
      std::vector<int32_t> ei, ej;
      for (size_t i = 0; i < N; ++i) {
        const double v[3] = {nrm(rng), nrm(rng), nrm(rng)};
        rodrigues(v, &Rgt[9 * i]);
      }
      for (size_t e = 0; e < N + N / 2; ++e) {
        const size_t i = e < N ? e : rng() % N;
        size_t j = e < N ? (e + 1) % N : rng() % N;
        if (j == i) j = (i + 2) % N;
        double M[9], noise[9], Mn[9];
        const double v[3] = {0.1 * nrm(rng), 0.1 * nrm(rng), 0.1 * nrm(rng)};
        mul(&Rgt[9 * i], true, &Rgt[9 * j], M);
        rodrigues(v, noise);
        mul(M, false, noise, Mn);
        ei.push_back((int32_t)i);
        ej.push_back((int32_t)j);
        Rt.insert(Rt.end(), Mn, Mn + 9);
        w.push_back(uw(rng));
      }
      MI355::RotationAveraging prob(ctx, N, ei.size(), ei.data(), ej.data(), Rt.data(), w.data());
      Riemannian::TNTParams<double> params;
      params.gradient_tolerance = 1e-9;
      params.relative_decrease_tolerance = 0;
      params.stepsize_tolerance = 0;
      std::optional<Riemannian::LinearOperator<DeviceVector, DeviceVector>> pc = prob.preconditioner();
      auto res = Riemannian::TNT<DeviceVector, DeviceVector>(prob.objective(), prob.quadratic_model(), prob.metric(),
                                                             prob.retraction(), DeviceVector(ctx, Rgt.data(), 9 * N), pc, params);
      std::printf("TNT: %zu outer iterations, |grad| = %.1e\n", res.inner_iterations.size(), res.gradfx_norm);
      ok = report("ring with chords, noise 0.1", prob, res.x, true) && ok;
    }
    {  // (b) the winding on the N-cycle
      std::vector<double> R(9 * N), Rt(9 * N, 0.0), w(N, 1.0);
      std::vector<int32_t> ei(N), ej(N);
      for (size_t i = 0; i < N; ++i) {
        const double v[3] = {0, 0, 2 * M_PI * (double)i / (double)N};
        rodrigues(v, &R[9 * i]);
        Rt[9 * i] = Rt[9 * i + 4] = Rt[9 * i + 8] = 1.0;
        ei[i] = (int32_t)i;
        ej[i] = (int32_t)((i + 1) % N);
      }
      MI355::RotationAveraging prob(ctx, N, N, ei.data(), ej.data(), Rt.data(), w.data());
      std::printf("closed form: lambda_min = 2 cos(2 pi / N) - 2 = %.6e\n", 2 * std::cos(2 * M_PI / (double)N) - 2);
      ok = report("winding on the cycle", prob, DeviceVector(ctx, R.data(), 9 * N), false) && ok;
    }
    return ok ? 0 : 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 2;
  }
}
