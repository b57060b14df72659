// pgo_pack.h -- the host-side layout of the joint pose-graph problem on SE(3)^N (pgo.hip: mi_pgo_create), as plain C++17
// that a host compiler takes on its own (tests/test_cpu_pgo_pack.py, tests/cpp/sanitize_pgo_pack.cpp): no HIP types, no
// device.
//
//     f(R, t) = 1/2 sum_e kappa_e | R_j - R_i Rt_e |_F^2  +  1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2,   e = (i -> j)
//
// What is built here is the node-centric incidence layout of so3_pack.h (so3_pack_graph: SELL-64-sigma slices, perm, nbr;
// so3_slot_words: one word per slot, edge << 1 | (the slot's node is the FIRST node of the edge)) with four per-slot
// measurement streams, component-major per slice entry -- component c of slot (k, lane) of a stream of C components at
// (k * C + c) * 64 + lane -- and zero on padding slots:
//     rinc   (9)  the rotation measurement as the slot's node uses it: Rt_e at the second node, Rt_e' at the first
//                 (the 9-component form of Sinc; there is no quaternion form here)
//     tinc   (3)  tt_e
//     kinc   (1)  kappa_e
//     tauinc (1)  tau_e
// Every stream holds at least one element.  No kernel of pgo.hip walks the edges, so there is no per-edge stream.
// Refused (1, with the reason in err): N outside [1, 2^31 - 1), E >= 2^31, an end point outside [0, N), a self-loop, a
// non-finite tt, a tau that is negative or not finite.  kappa and Rt are taken as mi_so3n_create takes w and Rt: as given.
#pragma once

#include <cmath>

#include "so3_pack.h"

namespace mi {

struct PgoPack {
  size_t N = 0, E = 0, nslices = 0, nnzb = 0, padded = 0;
  std::vector<long long> slice_ptr;  // nslices + 1
  std::vector<int> perm, nbr;        // nslices * 64; padded
  std::vector<uint32_t> slot;        // padded (at least one element, as the four below)
  std::vector<double> rinc, tinc;    // padded * 9, padded * 3
  std::vector<double> kinc, tauinc;  // padded each
};

inline int pgo_pack(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *tt,
                    const double *kappa, const double *tau, PgoPack &out, std::string &err) {
  if (!(N > 0 && N < (size_t)INT32_MAX)) return err = "bad number of poses", 1;
  if (!(E < ((size_t)1 << 31))) return err = "bad number of edges", 1;
  for (size_t e = 0; e < E; ++e) {
    if (!(ei[e] >= 0 && (size_t)ei[e] < N && ej[e] >= 0 && (size_t)ej[e] < N))
      return err = "edge " + std::to_string(e) + " has an end point outside [0, N)", 1;
    if (ei[e] == ej[e]) return err = "edge " + std::to_string(e) + " is a self-loop", 1;
    if (!(std::isfinite(tt[3 * e]) && std::isfinite(tt[3 * e + 1]) && std::isfinite(tt[3 * e + 2])))
      return err = "edge " + std::to_string(e) + " has a non-finite translation", 1;
    if (!(tau[e] >= 0 && std::isfinite(tau[e]))) return err = "edge " + std::to_string(e) + " has a negative or non-finite weight", 1;
  }
  So3Graph G;
  if (so3_pack_graph(N, E, ei, ej, false, G, err)) return 1;
  const size_t padded = G.padded;
  so3_slot_words(G, out.slot);
  if (out.slot.empty()) out.slot.assign(1, 0u);
  out.rinc.assign(std::max<size_t>(1, padded * 9), 0.0);
  out.tinc.assign(std::max<size_t>(1, padded * 3), 0.0);
  out.kinc.assign(std::max<size_t>(1, padded), 0.0);
  out.tauinc.assign(std::max<size_t>(1, padded), 0.0);
  for (size_t s = 0; s < G.nslices; ++s)
    for (long long k = G.slice_ptr[s]; k < G.slice_ptr[s + 1]; ++k)
      for (int lane = 0; lane < 64; ++lane) {
        const size_t e0 = (size_t)k * 64 + lane;
        const int e = G.edge[e0];
        if (e < 0) continue;
        const double *M = Rt + 9 * (size_t)e;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c)
            out.rinc[((size_t)k * 9 + r * 3 + c) * 64 + lane] = G.dir[e0] > 0 ? M[r * 3 + c] : M[c * 3 + r];
        for (int c = 0; c < 3; ++c) out.tinc[((size_t)k * 3 + c) * 64 + lane] = tt[3 * (size_t)e + c];
        out.kinc[e0] = kappa[e];
        out.tauinc[e0] = tau[e];
      }
  out.N = N, out.E = E, out.nslices = G.nslices, out.nnzb = G.nnzb, out.padded = padded;
  out.slice_ptr = std::move(G.slice_ptr), out.perm = std::move(G.perm), out.nbr = std::move(G.nbr);
  return 0;
}

}  // namespace mi
