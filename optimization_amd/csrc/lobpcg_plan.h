// lobpcg_plan.h -- the decisions of lobpcg.hip's host half (which kernel, which template selectors, what launch
// geometry, how the small coefficient matrix is packed) as plain C++17 that a host compiler takes on its own
// (tests/test_cpu_lobpcg_plan.py through the mi_debug_lobpcg_* entries, tests/cpp/sanitize_lobpcg_plan.cpp): no HIP
// types, no device pointers -- alignment comes in as a flag.  The launch code reads these structs and computes nothing.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace mi {

// (lobpcg.hip and mi_internal.h assert that these are the kernels' own constants)
constexpr int kPlanGramRows = 32, kPlanGramLd = 34, kPlanGramWaves = 8;  // kGramRows, kGramLd, kGramWaves
constexpr int kPlanGdH = 1;                                               // kGdH
constexpr int kPlanSwRows = 512, kPlanMaxRows = 1024;                     // kSwRows, kMaxRows
constexpr int kPlanMaxSteps = 18;                                         // StepBases::p

inline bool aligned_to(size_t bytes, std::initializer_list<uintptr_t> addrs) {  // (a null pointer counts as aligned)
  return std::all_of(addrs.begin(), addrs.end(), [bytes](uintptr_t a) { return a % bytes == 0; });
}

// ---- the one eligibility rule of the LDS-free Gram kernels ------------------------------------------------------------
// A lane loads four consecutive rows of a column with one 32-byte load: m % 4 == 0 and every column block 32-byte
// aligned; the accumulators of a wave hold at most 5 x 5 tiles: k <= 80; and the grid is one wave per row range, so
// there must be at least one whole row step (min_rows), or the launch would be empty:
constexpr size_t kGramDirectMinRows = 16 * (size_t)kPlanGdH;  // k_gram_direct: a pipeline step is kGdH blocks of 16 rows;
                                                              // the rows past the last whole step go to k_gram_tail
constexpr size_t kGramPairMinRows = 16;  // k_gram_pair_sym: steps of 16 rows; the m % 16 leftover rows are a masked step
                                         // of one of the waves, which exists only if a whole step does
inline bool gram_direct_ok(size_t m, int k, bool aligned32, size_t min_rows) {
  return k <= 80 && m % 4 == 0 && aligned32 && m >= min_rows;
}

// ---- G = S'T (gram_impl) ---------------------------------------------------------------------------------------------
struct GramPlan {
  bool ok;       // false: a split right-hand side on a shape the direct kernel does not take
  bool direct;   // k_gram_direct<T, same> (+ k_gram_tail) : k_gram<same, aligned, tpw>
  bool same, aligned, tail;
  int T, tpw;    // T = min(kapad / 16, 5); tpw = tiles per wave of k_gram, 1..5
  int occ;       // direct: waves per SIMD (0 for k_gram)
  size_t nwaves, nb, mfull, lds;  // nb partial Grams; mfull rows in whole pipeline steps; dynamic LDS of k_gram
};
// same_panel: S and T are one panel; split: T = [T1 | T2]; aligned16 / aligned32: every panel involved
inline GramPlan gram_plan(size_t m, int ka, int kb, bool same_panel, bool split, bool aligned16, bool aligned32,
                          int num_cu) {
  GramPlan p{};
  const int kapad = (ka + 15) / 16 * 16, kbpad = (kb + 15) / 16 * 16;
  p.same = !split && same_panel && ka == kb;
  p.aligned = m % 2 == 0 && aligned16;
  p.direct = ka == kb && gram_direct_ok(m, ka, aligned32, kGramDirectMinRows);
  p.ok = !split || p.direct;
  p.T = std::min(kapad / 16, 5);
  p.mfull = m - m % (16 * kPlanGdH);
  if (p.direct) {  // one partial per wave + one for the leftover rows
    // two waves per SIMD where the registers allow it (k <= 48, and k <= 80 when S == T), else one
    p.occ = (kapad <= 48 || p.same) ? 2 : 1;
    p.nwaves = (std::min<size_t>(4 * (size_t)p.occ * num_cu, p.mfull / (16 * kPlanGdH)) + 3) / 4 * 4;
    p.tail = p.mfull < m;
    p.nb = p.nwaves + (p.tail ? 1 : 0);
  } else {  // rows per workgroup: a multiple of the 32-row tile, ~3 workgroups per CU
    p.nb = std::max<size_t>(1, std::min<size_t>(3 * (size_t)num_cu, (m + kPlanGramRows - 1) / kPlanGramRows));
    const int ta = kapad / 16, tb = kbpad / 16, ntiles = p.same ? ta * (ta + 1) / 2 : ta * tb;
    p.tpw = std::min((ntiles + kPlanGramWaves - 1) / kPlanGramWaves, 5);
    p.lds = (size_t)(p.same ? kapad : kapad + kbpad) * kPlanGramLd * sizeof(double);
  }
  return p;
}

// ---- (S'T, S'S) or (S'A(S), S'B(S)), upper block triangles (gram_pair_sym_direct) -------------------------------------
struct GramPairPlan {
  int T;      // k_gram_pair_sym<T, half, pair>
  bool half;  // the last tile column at most half full: the two Grams share it
  bool pair;  // both Grams from one launch (false, the generalized problem: one launch each)
  int occ;    // resident waves per SIMD: 62+16 / 132+48 registers at 1 / 2 tiles, then > 256
  size_t nwaves, mfull;  // (the leftover rows are a step of one of the waves: nwaves partial Grams)
};
inline GramPairPlan gram_pair_plan(size_t m, int k, bool pair, bool no_gram_half, int num_cu) {
  GramPairPlan p{};
  const int kpad = (k + 15) / 16 * 16;
  p.T = std::min(kpad / 16, 5);
  p.pair = pair;
  p.half = pair && k % 16 >= 1 && k % 16 <= 8 && !no_gram_half;
  p.mfull = m - m % 16;
  p.occ = kpad <= 32 ? 2 : 1;
  p.nwaves = (std::min<size_t>(4 * (size_t)p.occ * num_cu, p.mfull / 16) + 3) / 4 * 4;
  return p;
}

// ---- Y = S C (update2_impl) ------------------------------------------------------------------------------------------
// The matrix-pipe kernel takes the whole-iteration update -- 33..48 output columns (one chunk of 48) from a basis that
// cuts into 6..18 steps of four columns, none straddling two blocks; every other shape goes through the VALU kernels in
// chunks of 48 / 24 / 16 / 8 output columns (widest chunk that fits what is left: one pass over S per chunk).
struct UpdateStep {
  int block, first;  // the step's four columns: first .. first + 3 of this block
  int logical[4];    // basis column behind each of the four coefficient rows; -1: a zero row (a block's last step, when
                     // the width is no multiple of four, is its LAST four columns: the overlap is masked)
};
struct UpdateChunk {
  int c0, width;
  size_t off;  // of the chunk's coefficients in Ct
};
struct UpdatePlan {
  bool all_mfma = false;
  int ks = 0, kc = 0;
  std::vector<UpdateStep> steps;    // all_mfma only
  std::vector<UpdateChunk> chunks;  // all_mfma: the one chunk {0, 48, 0}
  size_t total = 0;                 // doubles of Ct
};
inline UpdatePlan update_plan(size_t m, int kc, const int *cols, int nblocks, bool no_update_mfma) {
  UpdatePlan p;
  p.kc = kc;
  for (int bi = 0; bi < nblocks; ++bi) p.ks += cols[bi];
  p.all_mfma = kc > 32 && kc <= 48 && m >= 16 && !no_update_mfma;
  for (int bi = 0, start = 0; bi < nblocks && p.all_mfma; start += cols[bi++]) {
    const int cb = cols[bi];
    if (cb < 4) p.all_mfma = false;
    for (int j = 0; 4 * j < cb && p.all_mfma; ++j) {
      if ((int)p.steps.size() == kPlanMaxSteps) { p.all_mfma = false; break; }
      const int first = std::min(4 * j, cb - 4);
      UpdateStep s{bi, first, {}};
      for (int q = 0; q < 4; ++q) s.logical[q] = first + q >= 4 * j ? start + first + q : -1;
      p.steps.push_back(s);
    }
  }
  if (p.steps.size() < 6) p.all_mfma = false;
  if (p.all_mfma) {
    p.chunks.push_back({0, 48, 0});
    p.total = p.steps.size() * 4 * 48;
    return p;
  }
  p.steps.clear();
  for (int c0 = 0; c0 < kc;) {
    const int left = kc - c0;
    const int width = left > 32 ? 48 : (left > 16 ? 24 : (left > 8 ? 16 : 8));  // 48 = X and P of one iteration
    p.chunks.push_back({c0, width, p.total});
    p.total += (size_t)p.ks * width;
    c0 += width;
  }
  return p;
}
// Ct of the plan from the column-major ks x kc matrix C (leading dimension ldc >= ks).  Matrix-pipe form: one row of 48
// per (step, column of the step), zero for masked rows; VALU form: per chunk ks x width row-major by basis column,
// packed back to back.  Zero-padded past kc either way.
inline std::vector<double> pack_update_coefficients(const UpdatePlan &p, const double *C_host, int ldc) {
  std::vector<double> Ct(p.total, 0.0);
  if (p.all_mfma) {
    for (size_t s = 0; s < p.steps.size(); ++s)
      for (int q = 0; q < 4; ++q) {
        const int sidx = p.steps[s].logical[q];
        if (sidx < 0) continue;
        for (int c = 0; c < p.kc; ++c) Ct[(s * 4 + q) * 48 + c] = C_host[(size_t)c * ldc + sidx];
      }
    return Ct;
  }
  for (const UpdateChunk &ch : p.chunks)
    for (int s = 0; s < p.ks; ++s)
      for (int c = 0; c < ch.width && ch.c0 + c < p.kc; ++c)
        Ct[ch.off + (size_t)s * ch.width + c] = C_host[(size_t)(ch.c0 + c) * ldc + s];
  return Ct;
}

// ---- the plane-sweep panel product (spmm_sweep_launch) ----------------------------------------------------------------
// D: the matrix's pure far stride in rows (one plane), n rows, k columns in passes of 8.  A plane is cut into tiles of
// kSwRows rows, the planes into zsegs segments of zs planes; one workgroup per (tile, segment) and pass, and one partial
// row per workgroup of a pass: xgrid = tiles * zsegs <= kMaxRows.
inline size_t sweep_tiles(size_t D) { return (D + kPlanSwRows - 1) / kPlanSwRows; }
// what spmm_sweep_ok asks besides the matrix's form: a plane of more than kMaxRows tiles has no such grid (window form)
inline bool sweep_fits(size_t D) { return D > 0 && sweep_tiles(D) <= (size_t)kPlanMaxRows; }
struct SweepPlan {
  bool ok;  // sweep_fits(D)
  int tiles, nst, npass, zsegs, zs, xgrid;
};
inline SweepPlan sweep_plan(size_t D, size_t n, int k, int num_cu, int sweep_zsegs) {
  SweepPlan p{};
  p.ok = sweep_fits(D);
  if (D == 0) return p;
  p.tiles = (int)sweep_tiles(D);
  p.nst = (int)((n + D - 1) / D);
  p.npass = (k + 7) / 8;
  // z-segments: enough workgroups to fill the chip twice over in one launch, at most kMaxRows partial rows, and not so
  // short that a segment's start-up (three plane-tiles loaded for zs computed) weighs more than ~20 %
  int zsegs = sweep_zsegs > 0 ? sweep_zsegs : (4 * num_cu + p.tiles * p.npass - 1) / (p.tiles * p.npass);
  zsegs = std::max(1, std::min(zsegs, std::min(p.nst / 12 > 0 ? p.nst / 12 : 1, kPlanMaxRows / p.tiles)));
  p.zs = (p.nst + zsegs - 1) / zsegs;
  p.zsegs = (p.nst + p.zs - 1) / p.zs;
  p.xgrid = p.tiles * p.zsegs;
  return p;
}

}  // namespace mi
