// sanitize_so3_pack.cpp -- the host-side layout of an SO(3)^N problem (optimization_amd/csrc/so3_pack.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, leak check included: the graphs of tests/test_cpu_so3n_pack.py in kind
// (sizes around the 64-lane slice and the 1024-node window, no edges, an isolated node, parallel edges, zero and negative
// weights, a reflection, both switches) and every refused problem, each packed into a fresh So3Pack and into one that
// held another problem before.  Built beside sanitize_host by optimization_amd/build.py build_sanitize() and run on
// the CPU; any report aborts with a non-zero exit code.
#include <cstdio>
#include <random>

#include "so3_pack.h"

static int fail(const char *what, size_t N) {
  std::fprintf(stderr, "sanitize_so3_pack: %s failed at N = %zu\n", what, N);
  return 1;
}

int main() {
  std::mt19937_64 gen(7);
  std::uniform_real_distribution<double> u(0.5, 2.0);
  mi::So3Pack reused;
  std::string err;
  for (size_t N : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)1025, (size_t)2049}) {
    // a ring over the nodes but one, chords, the first edge once more backwards
    std::vector<int32_t> ei, ej;
    const size_t iso = N / 2, n = N >= 4 ? N - 1 : N;
    auto node = [&](size_t k) { return (int32_t)(N >= 4 && k >= iso ? k + 1 : k); };
    if (n >= 3)
      for (size_t k = 0; k < n; ++k) ei.push_back(node(k)), ej.push_back(node((k + 1) % n));
    else if (n == 2)
      ei.push_back(0), ej.push_back(1);
    if (n >= 4) {
      for (size_t c = 0; c < N / 2; ++c) {
        const size_t a = gen() % n, b = gen() % n;
        if (a != b) ei.push_back(node(a)), ej.push_back(node(b));
      }
      ei.push_back(ej[0]), ej.push_back(ei[0]);
    }
    const size_t E = ei.size();
    std::vector<double> Rt(9 * E, 0.0), w(E);
    for (size_t e = 0; e < E; ++e) {
      const double t = u(gen), c = std::cos(t), s = std::sin(t);  // a rotation about the axis e % 3
      const int a = (int)(e % 3), b = (a + 1) % 3, d = (a + 2) % 3;
      double *M = Rt.data() + 9 * e;
      M[4 * a] = 1, M[4 * b] = c, M[4 * d] = c, M[3 * b + d] = -s, M[3 * d + b] = s;
      w[e] = u(gen);
    }
    if (E > 3) w[3] = 0.0;
    for (int variant = 0; variant < 3; ++variant) {  // plain, a negative weight, a reflection
      std::vector<double> Rv = Rt, wv = w;
      if (E && variant == 1) wv[E / 2] = -0.25;
      if (E && variant == 2) Rv[9 * (E / 3) + 4 * ((E / 3 + 2) % 3)] *= -1;
      for (int sw = 0; sw < 4; ++sw) {
        mi::So3Pack fresh;
        for (mi::So3Pack *P : {&fresh, &reused}) {
          if (mi::so3_pack(N, E, ei.data(), ej.data(), Rv.data(), wv.data(), sw & 1, sw & 2, *P, err)) return fail("so3_pack", N);
          if (P->padded != 64 * (size_t)P->slice_ptr[P->nslices] || P->nnzb != 2 * E) return fail("counts", N);
          if (P->sinc_quat != (!(sw & 1) && !(E && variant == 2)) || P->w_nonneg != !(E && variant == 1)) return fail("forms", N);
        }
      }
    }
    // refused: an end point out of range at either end, a self-loop -- the output may hold anything, but nothing leaks
    if (E) {
      const int32_t bad[4][2] = {{-1, 0}, {0, (int32_t)N}, {(int32_t)N, 0}, {0, 0}};
      for (const auto &b : bad) {
        std::vector<int32_t> bi = ei, bj = ej;
        bi[E - 1] = b[0], bj[E - 1] = b[1];
        if (mi::so3_pack(N, E, bi.data(), bj.data(), Rt.data(), w.data(), false, false, reused, err) != 1) return fail("refusal", N);
        if (err != "edge " + std::to_string(E - 1) + " has invalid endpoints") return fail("message", N);
      }
    }
  }
  for (size_t N : {(size_t)0, (size_t)INT32_MAX, (size_t)1 << 40})
    if (mi::so3_pack(N, 0, nullptr, nullptr, nullptr, nullptr, false, false, reused, err) != 1 || err != "bad number of rotations")
      return fail("refusal", N);
  std::printf("sanitize_so3_pack: ok\n");
  return 0;
}
