// examples/spectral_rotation_averaging.cpp -- rotation averaging without a start point of one's own:
//   initialise  RotationAveraging::spectral_initialization: the three lowest eigenvectors of the connection Laplacian by
//               the device LOBPCG, every 3 x 3 block rounded to the nearest rotation;
//   solve       Riemannian::TNT from that point;
//   certify     RotationAveraging::certify at what TNT reaches.
// The problem is the N-cycle with identity measurements, whose winding R_i = rot_z(2 pi i / N) is a critical point that a
// local solver started there never leaves (examples/certify_rotation_averaging.cpp refuses it).  The spectral point is the
// global minimiser itself: f = 0, certified.
//
//   (built by optimization_amd/build.py: build_harness() into examples/bin/; by hand:)
//   g++ -std=c++17 -O2 -I optimization_amd/include -I include examples/spectral_rotation_averaging.cpp \
//       -L optimization_amd -lmi355opt -Wl,-rpath,$PWD/optimization_amd -o spectral_rotation_averaging
//   ./spectral_rotation_averaging [N]        (rotations, default 200)
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <vector>

#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNT.h"

using namespace Optimization;
using MI355::DeviceVector;

int main(int argc, char **argv) {
  const size_t N = argc > 1 ? (size_t)std::atol(argv[1]) : 200;
  if (N < 5) return 2;
  try {
    MI355::Context ctx(0);
    std::vector<double> Rt(9 * N, 0.0), w(N, 1.0);
    std::vector<int32_t> ei(N), ej(N);
    for (size_t i = 0; i < N; ++i) {
      Rt[9 * i] = Rt[9 * i + 4] = Rt[9 * i + 8] = 1.0;
      ei[i] = (int32_t)i;
      ej[i] = (int32_t)((i + 1) % N);
    }
    MI355::RotationAveraging prob(ctx, N, N, ei.data(), ej.data(), Rt.data(), w.data());
    const MI355::SpectralResult s = prob.spectral_initialization();
    std::printf("spectral initialisation: %zu LOBPCG iterations (%s), eigenvalues %.3e %.3e %.3e\n", s.iterations,
                s.converged ? "converged" : "NOT converged", s.eigenvalues[0], s.eigenvalues[1], s.eigenvalues[2]);
    std::printf("    f(R0) = %.6e >= lower bound %.6e; %s, %zu degenerate blocks, separation %.3f\n", s.f, s.lower_bound,
                s.flipped ? "panel flipped" : "panel kept", s.degenerate, s.min_separation);
    Riemannian::TNTParams<double> params;
    params.gradient_tolerance = 1e-9;
    params.relative_decrease_tolerance = 0;
    params.stepsize_tolerance = 0;
    std::optional<Riemannian::LinearOperator<DeviceVector, DeviceVector>> pc = prob.preconditioner();
    auto res = Riemannian::TNT<DeviceVector, DeviceVector>(prob.objective(), prob.quadratic_model(), prob.metric(),
                                                           prob.retraction(), s.R, pc, params);
    std::printf("TNT: %zu outer iterations, |grad| = %.1e\n", res.inner_iterations.size(), res.gradfx_norm);
    const MI355::CertifyResult c = prob.certify(res.x);
    std::printf("certify: f = %.6e, lambda_min = %.6e (safe %.6e, eta %.1e) after %zu LOBPCG iterations  =>  %s\n", c.f,
                c.lambda_min, c.lambda_min_safe, c.eta, c.iterations,
                c.certified ? "CERTIFIED global minimiser" : "not certified");
    return s.converged && c.converged && c.certified ? 0 : 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 2;
  }
}
