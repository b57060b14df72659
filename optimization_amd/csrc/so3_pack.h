// so3_pack.h -- the host-side layout of an SO(3)^N problem (so3.hip: mi_so3n_create; the layout comment is at the top of
// that file), as plain C++17 that a host compiler takes on its own (tests/test_cpu_so3n_pack.py,
// tests/cpp/sanitize_so3_pack.cpp): no HIP types, no device.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace mi {

constexpr size_t kSo3Window = 1024;  // sigma: the nodes one workgroup pass owns (mi_internal.h: kBlock)

struct So3Pack {
  size_t N = 0, E = 0, nslices = 0, nnzb = 0, padded = 0;
  bool sinc_quat = false;  // the measurement streams hold unit quaternions (every measurement is a rotation to rounding)
  bool w_nonneg = true;
  // what the model assembly streams
  std::vector<long long> slice_ptr;  // nslices + 1
  std::vector<int> perm;             // nslices * 64: node owned by (slice, lane), -1: padding lane of the last window
  std::vector<int> nbr;              // padded: neighbour node (padding: own node)
  std::vector<double> sinc, winc;    // padded * (4 | 9) component-major per slice entry, padded (at least one element each)
  // what the least-squares view uploads later
  std::vector<int32_t> h_ij;         // 2E: (i, j) per edge
  std::vector<double> h_Se, h_w;     // E * (4 | 9) component-major measurement stream (as sinc_quat says); E weights
  std::vector<uint32_t> h_slot;      // padded: edge << 1 | (the slot's node is the first node of the edge); padding 0
};

// every measurement is a rotation to rounding: |S'S - I| <= 1e-13 entry by entry, det > 0
inline bool so3_all_rotations(size_t E, const double *Rt) {
  for (size_t e = 0; e < E; ++e) {
    const double *M = Rt + 9 * e;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double d = M[a] * M[b] + M[3 + a] * M[3 + b] + M[6 + a] * M[6 + b] - (a == b ? 1.0 : 0.0);
        if (!(std::fabs(d) <= 1e-13)) return false;
      }
    const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    if (!(det > 0)) return false;
  }
  return true;
}

// Rotation (row-major) -> unit quaternion (w, x, y, z): Shepperd's branch on the largest of (trace, m00, m11, m22).
// The slot stream and the edge stream both go through here: a second node's slot and its edge expand to the same bits.
// (inlined into both loops, as the lambda it was: 4.5e6 calls at the cfg3 size)
__attribute__((always_inline)) inline void so3_rotation_to_quat(const double *M, double *qv) {
  const double tr = M[0] + M[4] + M[8];
  double w, x, y, z;
  if (tr >= M[0] && tr >= M[4] && tr >= M[8]) {
    w = 1 + tr; x = M[7] - M[5]; y = M[2] - M[6]; z = M[3] - M[1];
  } else if (M[0] >= M[4] && M[0] >= M[8]) {
    w = M[7] - M[5]; x = 1 + M[0] - M[4] - M[8]; y = M[1] + M[3]; z = M[2] + M[6];
  } else if (M[4] >= M[8]) {
    w = M[2] - M[6]; x = M[1] + M[3]; y = 1 - M[0] + M[4] - M[8]; z = M[5] + M[7];
  } else {
    w = M[3] - M[1]; x = M[2] + M[6]; y = M[5] + M[7]; z = 1 - M[0] - M[4] + M[8];
  }
  const double nrm = std::sqrt(w * w + x * x + y * y + z * z);
  qv[0] = w / nrm; qv[1] = x / nrm; qv[2] = y / nrm; qv[3] = z / nrm;
}

// The graph part of the layout, shared with pgo_trans_pack.h: the SELL-64-sigma slices, the node of every lane, and for
// every slot its neighbour, its edge (-1: padding) and whether the slot's node is the second (+1) or the first (-1) node.
struct So3Graph {
  size_t nslices = 0, nnzb = 0, padded = 0;
  std::vector<long long> slice_ptr;
  std::vector<int> perm, nbr, edge;
  std::vector<signed char> dir;
};
// 0, or 1 with the reason in err.  sort_nbr: see so3_pack.
inline int so3_pack_graph(size_t N, size_t E, const int32_t *ei, const int32_t *ej, bool sort_nbr, So3Graph &out, std::string &err) {
  if (!(N > 0 && N < (size_t)INT32_MAX)) return err = "bad number of rotations", 1;
  for (size_t e = 0; e < E; ++e)
    if (!(ei[e] >= 0 && (size_t)ei[e] < N && ej[e] >= 0 && (size_t)ej[e] < N && ei[e] != ej[e]))
      return err = "edge " + std::to_string(e) + " has invalid endpoints", 1;
  // incidence lists: node -> (edge, direction), in edge order
  std::vector<std::vector<int>> lists(N);
  for (size_t e = 0; e < E; ++e) {
    lists[(size_t)ej[e]].push_back((int)e + 1);     // second node: +(e+1)
    lists[(size_t)ei[e]].push_back(-((int)e + 1));  // first node: -(e+1)
  }
  if (sort_nbr)
    for (size_t i = 0; i < N; ++i)
      std::stable_sort(lists[i].begin(), lists[i].end(), [&](int a, int b) {
        const int ea = std::abs(a) - 1, eb = std::abs(b) - 1;
        const int ja = a > 0 ? ei[ea] : ej[ea], jb = b > 0 ? ei[eb] : ej[eb];
        return ja < jb;
      });
  // SELL-64-sigma: inside each window the nodes are ordered by descending degree (stable), so a slice's 64 nodes have
  // near-equal degree and the padding of an irregular pose graph drops from ~1.66x to ~1.05x of the incidences.  The
  // window is a contiguous node range, so x_i loads / h_i stores stay inside one 24 KB span per workgroup pass; tangent
  // vectors keep the caller's node order.
  const size_t nslices = (N + 63) / 64;
  std::vector<int> &perm = out.perm;
  perm.assign(nslices * 64, -1);
  for (size_t w0 = 0; w0 < N; w0 += kSo3Window) {
    const size_t w1 = std::min(N, w0 + kSo3Window);
    std::vector<int> ids(w1 - w0);
    for (size_t i = w0; i < w1; ++i) ids[i - w0] = (int)i;
    std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return lists[(size_t)a].size() > lists[(size_t)b].size(); });
    for (size_t i = w0; i < w1; ++i) perm[i] = ids[i - w0];
  }
  std::vector<long long> &sp = out.slice_ptr;
  sp.assign(nslices + 1, 0);
  for (size_t s = 0; s < nslices; ++s) {
    size_t wmax = 0;
    for (size_t l = s * 64; l < (s + 1) * 64; ++l)
      if (perm[l] >= 0) wmax = std::max(wmax, lists[(size_t)perm[l]].size());
    sp[s + 1] = sp[s] + (long long)wmax;
  }
  const size_t padded = (size_t)sp[nslices] * 64;
  std::vector<int> &nbr = out.nbr, &edge = out.edge;
  nbr.assign(padded, 0);
  edge.assign(padded, -1);
  std::vector<signed char> &dir = out.dir;
  dir.assign(padded, 0);
  size_t nnzb = 0;
  for (size_t s = 0; s < nslices; ++s)
    for (int lane = 0; lane < 64; ++lane) {
      const bool owned = perm[s * 64 + lane] >= 0;
      const size_t i = owned ? (size_t)perm[s * 64 + lane] : N - 1;
      for (long long k = 0; k < sp[s + 1] - sp[s]; ++k) {
        const size_t e0 = (size_t)(sp[s] + k) * 64 + lane;
        nbr[e0] = (int)i;
        if (owned && (size_t)k < lists[i].size()) {
          const int code = lists[i][(size_t)k];
          const int e = std::abs(code) - 1;
          edge[e0] = e;
          dir[e0] = code > 0 ? 1 : -1;
          nbr[e0] = code > 0 ? ei[e] : ej[e];
          ++nnzb;
        }
      }
    }
  out.nslices = nslices, out.nnzb = nnzb, out.padded = padded;
  return 0;
}
// the slot words of a graph: edge << 1 | (the slot's node is the first node of the edge); padding 0
inline void so3_slot_words(const So3Graph &G, std::vector<uint32_t> &words) {
  words.assign(G.padded, 0u);
  for (size_t e0 = 0; e0 < G.padded; ++e0)
    if (G.edge[e0] >= 0) words[e0] = ((uint32_t)G.edge[e0] << 1) | (G.dir[e0] < 0 ? 1u : 0u);
}

// 0, or 1 with the reason in err (an invalid argument).  no_quat: the measurements stay 3 x 3 matrices (SO3_NO_QUAT);
// sort_nbr: every node's incidences in ascending order of the NEIGHBOUR instead of edge order (experiment switch
// SO3_SORT_NBR, "incidences ordered in column phases": measured in DESIGN 5.1; changes the order of a row's sum).
inline int so3_pack(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w, bool no_quat,
                    bool sort_nbr, So3Pack &out, std::string &err) {
  So3Graph G;
  if (so3_pack_graph(N, E, ei, ej, sort_nbr, G, err)) return 1;
  const size_t nslices = G.nslices, padded = G.padded, nnzb = G.nnzb;
  out.perm = std::move(G.perm), out.slice_ptr = std::move(G.slice_ptr), out.nbr = std::move(G.nbr);
  const std::vector<long long> &sp = out.slice_ptr;
  const std::vector<int> &edge = G.edge;
  const std::vector<signed char> &dir = G.dir;
  // the measurement and weight of every incidence in slot order (k_so3_model streams them), the measurements as unit
  // quaternions when every one of them is a rotation to rounding (k_so3_model<., SQ>)
  const bool all_rot = !no_quat && so3_all_rotations(E, Rt);
  const int scomp = all_rot ? 4 : 9;
  out.sinc.assign(std::max<size_t>(1, padded * scomp), 0.0);
  out.winc.assign(std::max<size_t>(1, padded), 0.0);
  for (size_t s = 0; s < nslices; ++s)
    for (long long k = sp[s]; k < sp[s + 1]; ++k)
      for (int lane = 0; lane < 64; ++lane) {
        const size_t e0 = (size_t)k * 64 + lane;
        const int e = edge[e0];
        if (e < 0) continue;
        out.winc[e0] = w[e];
        double Sm[9];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) Sm[r * 3 + c] = dir[e0] > 0 ? Rt[9 * (size_t)e + r * 3 + c] : Rt[9 * (size_t)e + c * 3 + r];
        if (all_rot) {
          double qv[4];
          so3_rotation_to_quat(Sm, qv);
          for (int c = 0; c < 4; ++c) out.sinc[((size_t)k * 4 + c) * 64 + lane] = qv[c];
        } else {
          for (int c = 0; c < 9; ++c) out.sinc[((size_t)k * 9 + c) * 64 + lane] = Sm[c];
        }
      }
  // the edges in the caller's order: end points, weights, the measurement stream in the form of sinc, the slot words
  out.h_ij.resize(2 * E);
  out.h_w.assign(w, w + E);
  out.h_Se.resize(E * (size_t)scomp);
  out.w_nonneg = true;
  for (size_t e = 0; e < E; ++e) {
    out.h_ij[2 * e] = ei[e];
    out.h_ij[2 * e + 1] = ej[e];
    if (!(w[e] >= 0)) out.w_nonneg = false;
    double qv[9];
    if (all_rot) so3_rotation_to_quat(Rt + 9 * e, qv);
    else std::memcpy(qv, Rt + 9 * e, 9 * sizeof(double));
    for (int c = 0; c < scomp; ++c) out.h_Se[(size_t)c * E + e] = qv[c];
  }
  out.h_slot.assign(padded, 0u);
  if (E < ((size_t)1 << 31)) so3_slot_words(G, out.h_slot);
  out.N = N, out.E = E, out.nslices = nslices, out.nnzb = nnzb, out.padded = padded;
  out.sinc_quat = all_rot;
  return 0;
}

}  // namespace mi
