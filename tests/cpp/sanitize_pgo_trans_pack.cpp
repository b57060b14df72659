// sanitize_pgo_trans_pack.cpp -- the host-side layout of the pose-graph translation solve
// (optimization_amd/csrc/pgo_trans_pack.h) under AddressSanitizer + UndefinedBehaviorSanitizer, leak check included: the
// graphs of tests/test_cpu_pgo_trans_pack.py in kind (sizes around the 64-lane slice and the 1024-node window, no edges, an
// isolated node, parallel and two-way edges, zero weights, a node whose every weight is zero), every anchor kind (first,
// last, the isolated node, a node of the ragged last slice) and every refused problem, each packed into a fresh
// PgoTransPack and into one that held another problem before.  Built beside sanitize_host by optimization_amd/build.py
// build_sanitize() and run on the CPU; any report aborts with a non-zero exit code.
#include <cstdio>
#include <limits>
#include <random>

#include "pgo_trans_pack.h"

static int fail(const char *what, size_t N) {
  std::fprintf(stderr, "sanitize_pgo_trans_pack: %s failed at N = %zu\n", what, N);
  return 1;
}

int main() {
  std::mt19937_64 gen(11);
  std::uniform_real_distribution<double> u(0.5, 2.0);
  std::normal_distribution<double> g(0.0, 1.0);
  mi::PgoTransPack reused;
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
    std::vector<double> tt(3 * E), tau(E);
    for (size_t e = 0; e < E; ++e) {
      tau[e] = u(gen);
      for (int c = 0; c < 3; ++c) tt[3 * e + c] = g(gen);
    }
    for (size_t e = 0; e < E; e += 7) tau[e] = 0.0;
    if (N >= 4)  // every weight of node 1 exactly zero
      for (size_t e = 0; e < E; ++e)
        if (ei[e] == 1 || ej[e] == 1) tau[e] = 0.0;
    for (long long anchor : {(long long)0, (long long)N - 1, (long long)iso, (long long)(N - 1 - (N - 1) % 64)}) {
      mi::PgoTransPack fresh;
      for (mi::PgoTransPack *P : {&fresh, &reused}) {
        if (mi::pgo_trans_pack(N, E, ei.data(), ej.data(), tt.data(), tau.data(), anchor, *P, err)) return fail("pgo_trans_pack", N);
        if (P->padded != 64 * (size_t)P->slice_ptr[P->nslices] || P->nnzb != 2 * E) return fail("counts", N);
        if (P->rowptr.size() != N + 1 || (size_t)P->rowptr[N] != P->nnz || P->col.size() != P->nnz || P->val.size() != P->nnz)
          return fail("csr", N);
        if (P->dinv.size() != 3 * N || P->dinv[3 * (size_t)anchor] != 1.0) return fail("dinv", N);
        const int32_t a0 = P->rowptr[(size_t)anchor];
        if (P->rowptr[(size_t)anchor + 1] != a0 + 1 || P->col[(size_t)a0] != anchor || P->val[(size_t)a0] != 1.0) return fail("unit row", N);
        for (size_t k = 0; k < P->nnz; ++k)
          if (P->col[k] < 0 || (size_t)P->col[k] >= N) return fail("columns", N);
      }
    }
    // refused: the output may hold anything, but nothing leaks
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (long long anchor : {(long long)-1, (long long)N, (long long)1 << 40})
      if (mi::pgo_trans_pack(N, E, ei.data(), ej.data(), tt.data(), tau.data(), anchor, reused, err) != 1 ||
          err != "anchor " + std::to_string(anchor) + " is outside [0, N)")
        return fail("anchor refusal", N);
    if (E) {
      const std::string edge = "edge " + std::to_string(E - 1);
      const int32_t bad[3][2] = {{-1, 0}, {0, (int32_t)N}, {(int32_t)N, 0}};
      for (const auto &b : bad) {
        std::vector<int32_t> bi = ei, bj = ej;
        bi[E - 1] = b[0], bj[E - 1] = b[1];
        if (mi::pgo_trans_pack(N, E, bi.data(), bj.data(), tt.data(), tau.data(), 0, reused, err) != 1 ||
            err != edge + " has an end point outside [0, N)")
          return fail("end point refusal", N);
      }
      {
        std::vector<int32_t> bi = ei, bj = ej;
        bi[E - 1] = bj[E - 1] = 0;
        if (mi::pgo_trans_pack(N, E, bi.data(), bj.data(), tt.data(), tau.data(), 0, reused, err) != 1 || err != edge + " is a self-loop")
          return fail("self-loop refusal", N);
      }
      for (double v : {inf, -inf, nan}) {
        std::vector<double> bt = tt, bw = tau;
        bt[3 * (E - 1) + 1] = v;
        if (mi::pgo_trans_pack(N, E, ei.data(), ej.data(), bt.data(), tau.data(), 0, reused, err) != 1 ||
            err != edge + " has a non-finite translation")
          return fail("translation refusal", N);
        bw[E - 1] = v;
        if (mi::pgo_trans_pack(N, E, ei.data(), ej.data(), tt.data(), bw.data(), 0, reused, err) != 1 ||
            err != edge + " has a negative or non-finite weight")
          return fail("weight refusal", N);
      }
      std::vector<double> bw = tau;
      bw[E - 1] = -0.25;
      if (mi::pgo_trans_pack(N, E, ei.data(), ej.data(), tt.data(), bw.data(), 0, reused, err) != 1 ||
          err != edge + " has a negative or non-finite weight")
        return fail("weight refusal", N);
    }
  }
  for (size_t N : {(size_t)0, (size_t)INT32_MAX, (size_t)1 << 40})
    if (mi::pgo_trans_pack(N, 0, nullptr, nullptr, nullptr, nullptr, 0, reused, err) != 1 || err != "bad number of poses")
      return fail("refusal", N);
  std::printf("sanitize_pgo_trans_pack: ok\n");
  return 0;
}
