// pgo_trans_pack.h -- the host-side layout of the translation half of a pose graph (pgo_trans.hip: mi_pgo_trans_create),
// as plain C++17 that a host compiler takes on its own (tests/test_cpu_pgo_trans_pack.py,
// tests/cpp/sanitize_pgo_trans_pack.cpp): no HIP types, no device.
//
// With the rotations R fixed, the positions of edges e = (i -> j) with relative translation tt_e and weight tau_e >= 0 solve
//     min_t  1/2 sum_e tau_e | t_j - t_i - R_i tt_e |^2      <=>      L t = b(R),
//     L = the tau-weighted graph Laplacian (x) I_3,   b_i = sum_{e = (i -> .)} -tau_e R_i tt_e + sum_{e = (k -> i)} tau_e R_k tt_e
// in the gauge t_anchor = 0.  What is built here:
//   (1) the ANCHORED Laplacian L_a as CSR (int32 rowptr / col, fp64 val; columns ascending; parallel and two-way edges merged,
//       their weights summed in edge order): diagonal degtau_i = sum of tau_e over the incidences of i (edge order), off-diagonal
//       -(sum of tau_e between i and j).  The anchor's row and column are the unit row; a node of weighted degree 0 (no edge, or
//       every tau exactly 0) has the unit row as well (its position is not determined: it stays 0).  Entries that are exactly
//       zero are not stored, except on the diagonal.  Symmetric entry by entry (the same sums in the same order on both sides).
//   (2) dinv (3N): 1 / diagonal, each value three times -- the Jacobi preconditioner of L_a (x) I_3 on the N x 3 row-major field.
//   (3) the node-centric incidence layout of so3_pack.h (SELL-64-sigma slices, perm, nbr, one slot word edge << 1 | (the
//       slot's node is the FIRST node of the edge)) with two per-slot streams: tinc, the edge's tt_e, 3 components,
//       component-major like Sinc -- component c of slot (k, lane) at (k * 3 + c) * 64 + lane -- and tauinc, tau_e; 0 on
//       padding slots and on every slot of the anchor's and the zero-degree nodes' rows (their right-hand side is 0).
//   (4) the per-edge streams of the residual pass in the caller's edge order: (i, j), tt_e component-major (c * E + e), tau_e.
// Refused (1, with the reason in err): N outside [1, 2^31 - 1), E >= 2^31, an anchor outside [0, N), an end point outside
// [0, N), a self-loop, a non-finite tt, a tau that is negative or not finite, more than 2^31 - 1 stored entries.
// OUTSIDE THE METHOD AND NOT DETECTED: a graph with several components that carry edges.  Only the anchor's component is
// pinned; on the others L_a is singular but the system is consistent, and CG returns one of its solutions (the one with
// no component along the null space, from the zero start).
#pragma once

#include <cmath>

#include "so3_pack.h"

namespace mi {

struct PgoTransPack {
  size_t N = 0, E = 0, nslices = 0, nnzb = 0, padded = 0, nnz = 0, anchor = 0;
  // (1), (2)
  std::vector<int32_t> rowptr, col;
  std::vector<double> val, dinv;
  // (3)
  std::vector<long long> slice_ptr;  // nslices + 1
  std::vector<int> perm, nbr;        // nslices * 64; padded
  std::vector<uint32_t> slot;        // padded (at least one element, as the two below)
  std::vector<double> tinc, tauinc;  // padded * 3; padded
  // (4)
  std::vector<int32_t> e_ij;         // 2E
  std::vector<double> e_t, e_tau;    // 3E component-major; E
};

inline int pgo_trans_pack(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *tt, const double *tau,
                          long long anchor, PgoTransPack &out, std::string &err) {
  if (!(N > 0 && N < (size_t)INT32_MAX)) return err = "bad number of poses", 1;
  if (!(E < ((size_t)1 << 31))) return err = "bad number of edges", 1;
  if (!(anchor >= 0 && (size_t)anchor < N)) return err = "anchor " + std::to_string(anchor) + " is outside [0, N)", 1;
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
  // weighted degrees, every node's incidences in edge order (the order of its slots)
  std::vector<double> deg(N, 0.0);
  for (size_t e = 0; e < E; ++e) deg[(size_t)ei[e]] += tau[e], deg[(size_t)ej[e]] += tau[e];
  auto unit_row = [&](size_t i) { return i == (size_t)anchor || deg[i] == 0.0; };
  // (1), (2): rows in node order from the slots of each node (lane l of slice s, slots slice_ptr[s] ... in edge order)
  std::vector<size_t> lane_of(N);
  for (size_t l = 0; l < G.perm.size(); ++l)
    if (G.perm[l] >= 0) lane_of[(size_t)G.perm[l]] = l;
  out.rowptr.assign(N + 1, 0);
  out.col.clear(), out.val.clear();
  out.dinv.assign(3 * N, 1.0);
  std::vector<std::pair<int, double>> row;
  for (size_t i = 0; i < N; ++i) {
    row.clear();
    if (!unit_row(i)) {
      const size_t s = lane_of[i] / 64, lane = lane_of[i] % 64;
      for (long long k = G.slice_ptr[s]; k < G.slice_ptr[s + 1]; ++k) {
        const size_t e0 = (size_t)k * 64 + lane;
        if (G.edge[e0] < 0) break;  // (a node's incidences are its first slots)
        row.emplace_back(G.nbr[e0], tau[G.edge[e0]]);
      }
      std::stable_sort(row.begin(), row.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
    }
    bool diag_done = false;
    auto put_diag = [&] {
      out.col.push_back((int32_t)i);
      out.val.push_back(unit_row(i) ? 1.0 : deg[i]);
      diag_done = true;
    };
    for (size_t a = 0; a < row.size();) {
      size_t b = a;
      double sum = 0.0;
      for (; b < row.size() && row[b].first == row[a].first; ++b) sum += row[b].second;
      const size_t j = (size_t)row[a].first;
      a = b;
      if (j == (size_t)anchor || sum == 0.0) continue;  // the anchor's column; an explicit zero
      if (!diag_done && j > i) put_diag();
      out.col.push_back((int32_t)j);
      out.val.push_back(-sum);
    }
    if (!diag_done) put_diag();
    if (out.col.size() >= (size_t)INT32_MAX) return err = "the Laplacian has too many entries for int32 row pointers", 1;
    out.rowptr[i + 1] = (int32_t)out.col.size();
    if (!unit_row(i)) out.dinv[3 * i] = out.dinv[3 * i + 1] = out.dinv[3 * i + 2] = 1.0 / deg[i];
  }
  // (3)
  so3_slot_words(G, out.slot);
  if (out.slot.empty()) out.slot.assign(1, 0u);
  out.tinc.assign(std::max<size_t>(1, padded * 3), 0.0);
  out.tauinc.assign(std::max<size_t>(1, padded), 0.0);
  for (size_t s = 0; s < G.nslices; ++s)
    for (long long k = G.slice_ptr[s]; k < G.slice_ptr[s + 1]; ++k)
      for (int lane = 0; lane < 64; ++lane) {
        const size_t e0 = (size_t)k * 64 + lane;
        const int e = G.edge[e0];
        if (e < 0) continue;
        for (int c = 0; c < 3; ++c) out.tinc[((size_t)k * 3 + c) * 64 + lane] = tt[3 * (size_t)e + c];
        if (!unit_row((size_t)G.perm[s * 64 + lane])) out.tauinc[e0] = tau[e];
      }
  // (4)
  out.e_ij.resize(2 * E);
  out.e_t.resize(3 * E);
  out.e_tau.assign(tau, tau + E);
  for (size_t e = 0; e < E; ++e) {
    out.e_ij[2 * e] = ei[e], out.e_ij[2 * e + 1] = ej[e];
    for (int c = 0; c < 3; ++c) out.e_t[(size_t)c * E + e] = tt[3 * e + c];
  }
  out.N = N, out.E = E, out.nslices = G.nslices, out.nnzb = G.nnzb, out.padded = padded, out.nnz = out.col.size();
  out.anchor = (size_t)anchor;
  out.slice_ptr = std::move(G.slice_ptr), out.perm = std::move(G.perm), out.nbr = std::move(G.nbr);
  return 0;
}

}  // namespace mi
