// sanitize_pgo_pack.cpp -- the host-side layout of the joint pose-graph problem (optimization_amd/csrc/pgo_pack.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, leak check included: the graphs of tests/test_cpu_pgo_pack.py in kind
// (sizes around the 64-lane slice and the 1024-node window, no edges, an isolated node, parallel and two-way edges, zero
// weights, a node whose every weight is zero) and every refused problem, each packed into a fresh PgoPack and into one that
// held another problem before.  Built beside sanitize_host by optimization_amd/build.py build_sanitize() and run on the CPU;
// any report aborts with a non-zero exit code.
#include <cstdio>
#include <limits>
#include <random>

#include "pgo_pack.h"

static int fail(const char *what, size_t N) {
  std::fprintf(stderr, "sanitize_pgo_pack: %s failed at N = %zu\n", what, N);
  return 1;
}

int main() {
  std::mt19937_64 gen(13);
  std::uniform_real_distribution<double> u(0.5, 2.0);
  std::normal_distribution<double> g(0.0, 1.0);
  mi::PgoPack reused;
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
    std::vector<double> Rt(9 * E), tt(3 * E), kappa(E), tau(E);
    for (size_t e = 0; e < E; ++e) {
      kappa[e] = u(gen), tau[e] = u(gen);
      for (int c = 0; c < 9; ++c) Rt[9 * e + c] = g(gen);
      for (int c = 0; c < 3; ++c) tt[3 * e + c] = g(gen);
    }
    for (size_t e = 0; e < E; e += 7) tau[e] = 0.0;
    for (size_t e = 3; e < E; e += 5) kappa[e] = e % 2 ? 0.0 : -0.25;  // (kappa is taken as given)
    if (N >= 4)  // every weight of node 1 exactly zero
      for (size_t e = 0; e < E; ++e)
        if (ei[e] == 1 || ej[e] == 1) tau[e] = kappa[e] = 0.0;
    mi::PgoPack fresh;
    for (mi::PgoPack *P : {&fresh, &reused}) {
      if (mi::pgo_pack(N, E, ei.data(), ej.data(), Rt.data(), tt.data(), kappa.data(), tau.data(), *P, err)) return fail("pgo_pack", N);
      if (P->padded != 64 * (size_t)P->slice_ptr[P->nslices] || P->nnzb != 2 * E || P->N != N || P->E != E) return fail("counts", N);
      if (P->perm.size() != 64 * P->nslices || P->nbr.size() != P->padded) return fail("graph", N);
      if (P->slot.size() != std::max<size_t>(1, P->padded) || P->kinc.size() != P->slot.size() || P->tauinc.size() != P->slot.size() ||
          P->rinc.size() != std::max<size_t>(1, 9 * P->padded) || P->tinc.size() != std::max<size_t>(1, 3 * P->padded))
        return fail("streams", N);
      // every slot's streams against its edge, through the slot word
      for (size_t s = 0; s < P->nslices; ++s)
        for (long long k = P->slice_ptr[s]; k < P->slice_ptr[s + 1]; ++k)
          for (size_t lane = 0; lane < 64; ++lane) {
            const size_t e0 = (size_t)k * 64 + lane;
            if (P->nbr[e0] < 0 || (size_t)P->nbr[e0] >= N) return fail("neighbours", N);
            const int own = P->perm[s * 64 + lane];
            if (own < 0 || P->nbr[e0] == own) {  // padding
              if (P->slot[e0] != 0 || P->kinc[e0] != 0 || P->tauinc[e0] != 0) return fail("padding", N);
              continue;
            }
            const size_t e = P->slot[e0] >> 1;
            const bool first = P->slot[e0] & 1u;
            if (e >= E || (first ? ei[e] : ej[e]) != own || (first ? ej[e] : ei[e]) != P->nbr[e0]) return fail("slot words", N);
            if (P->kinc[e0] != kappa[e] || P->tauinc[e0] != tau[e]) return fail("weights", N);
            for (int c = 0; c < 3; ++c)
              if (P->tinc[((size_t)k * 3 + c) * 64 + lane] != tt[3 * e + c]) return fail("tinc", N);
            for (int r = 0; r < 3; ++r)
              for (int c = 0; c < 3; ++c)
                if (P->rinc[((size_t)k * 9 + r * 3 + c) * 64 + lane] != Rt[9 * e + (first ? c * 3 + r : r * 3 + c)]) return fail("rinc", N);
          }
    }
    // refused: the output may hold anything, but nothing leaks
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    if (E) {
      const std::string edge = "edge " + std::to_string(E - 1);
      const int32_t bad[3][2] = {{-1, 0}, {0, (int32_t)N}, {(int32_t)N, 0}};
      for (const auto &b : bad) {
        std::vector<int32_t> bi = ei, bj = ej;
        bi[E - 1] = b[0], bj[E - 1] = b[1];
        if (mi::pgo_pack(N, E, bi.data(), bj.data(), Rt.data(), tt.data(), kappa.data(), tau.data(), reused, err) != 1 ||
            err != edge + " has an end point outside [0, N)")
          return fail("end point refusal", N);
      }
      {
        std::vector<int32_t> bi = ei, bj = ej;
        bi[E - 1] = bj[E - 1] = 0;
        if (mi::pgo_pack(N, E, bi.data(), bj.data(), Rt.data(), tt.data(), kappa.data(), tau.data(), reused, err) != 1 ||
            err != edge + " is a self-loop")
          return fail("self-loop refusal", N);
      }
      for (double v : {inf, -inf, nan, -0.25}) {
        std::vector<double> bt = tt, bw = tau;
        bt[3 * (E - 1) + 1] = v;
        if (v != -0.25 && (mi::pgo_pack(N, E, ei.data(), ej.data(), Rt.data(), bt.data(), kappa.data(), tau.data(), reused, err) != 1 ||
                           err != edge + " has a non-finite translation"))
          return fail("translation refusal", N);
        bw[E - 1] = v;
        if (mi::pgo_pack(N, E, ei.data(), ej.data(), Rt.data(), tt.data(), kappa.data(), bw.data(), reused, err) != 1 ||
            err != edge + " has a negative or non-finite weight")
          return fail("weight refusal", N);
      }
    }
  }
  for (size_t N : {(size_t)0, (size_t)INT32_MAX, (size_t)1 << 40})
    if (mi::pgo_pack(N, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, reused, err) != 1 || err != "bad number of poses")
      return fail("refusal", N);
  std::printf("sanitize_pgo_pack: ok\n");
  return 0;
}
