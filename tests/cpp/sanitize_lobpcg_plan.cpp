// sanitize_lobpcg_plan.cpp -- the plans of the LOBPCG host layer (optimization_amd/csrc/lobpcg_plan.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, leak check included: the update plans and the coefficient packing of
// tests/test_cpu_lobpcg_plan.py (C held in a buffer of exactly ldc * kc doubles, so a read past it is a report), the
// shapes the matrix-pipe form refuses, the Gram and sweep plans on their grids with the refused ones.  Built beside
// sanitize_host by optimization_amd/build.py build_sanitize() and run on the CPU; any report aborts with a non-zero
// exit code.
#include <cstdio>
#include <random>

#include "lobpcg_plan.h"

static int fail(const char *what, long a, long b) {
  std::fprintf(stderr, "sanitize_lobpcg_plan: %s failed at (%ld, %ld)\n", what, a, b);
  return 1;
}

int main() {
  std::mt19937_64 gen(11);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  const std::vector<std::vector<int>> widths = {{72}, {48}, {24, 24, 24}, {24, 19, 17}, {24, 23, 23},
                                                {24, 25, 23} /* 19 steps */, {20} /* 5 steps */, {24, 3, 24} /* a block < 4 */};
  for (size_t wi = 0; wi < widths.size(); ++wi) {
    const std::vector<int> &cols = widths[wi];
    int ks = 0;
    for (int c : cols) ks += c;
    for (int kc : {1, 8, 9, 32, 33, 40, 48, 49, 96})
      for (int off = 0; off < 2; ++off)
        for (size_t m : {(size_t)15, (size_t)1000})
          for (int pad : {0, 5}) {
            const int ldc = ks + pad;
            std::vector<double> Cm((size_t)ldc * kc);
            for (double &v : Cm) v = u(gen);
            const mi::UpdatePlan p = mi::update_plan(m, kc, cols.data(), (int)cols.size(), off != 0);
            const std::vector<double> Ct = mi::pack_update_coefficients(p, Cm.data(), ldc);
            const bool may = kc > 32 && kc <= 48 && m >= 16 && !off && wi < 5;
            if (p.all_mfma != may || p.ks != ks || Ct.size() != p.total) return fail("form", (long)wi, kc);
            std::vector<double> back((size_t)ks * kc, 0.0);  // Ct scattered back: C(:ks, :kc), every entry exactly once
            size_t nonzero = 0;
            for (double v : Ct) nonzero += v != 0.0;
            if (p.all_mfma) {
              if (p.steps.size() < 6 || p.steps.size() > (size_t)mi::kPlanMaxSteps) return fail("steps", (long)wi, kc);
              for (size_t s = 0; s < p.steps.size(); ++s)
                for (int q = 0; q < 4; ++q) {
                  const int sidx = p.steps[s].logical[q];
                  if (sidx < -1 || sidx >= ks || p.steps[s].first + 4 > cols[p.steps[s].block]) return fail("step", (long)wi, kc);
                  for (int c = 0; c < kc && sidx >= 0; ++c) back[(size_t)c * ks + sidx] += Ct[(s * 4 + q) * 48 + c];
                }
            } else {
              if (!p.steps.empty()) return fail("steps", (long)wi, kc);
              int covered = 0;
              for (const mi::UpdateChunk &ch : p.chunks) {
                if (ch.c0 != covered || ch.off + (size_t)ks * ch.width > Ct.size()) return fail("chunk", (long)wi, kc);
                covered += ch.width;
                for (int s = 0; s < ks; ++s)
                  for (int c = 0; c < ch.width && ch.c0 + c < kc; ++c)
                    back[(size_t)(ch.c0 + c) * ks + s] += Ct[ch.off + (size_t)s * ch.width + c];
              }
              if (covered < kc) return fail("cover", (long)wi, kc);
            }
            for (int c = 0; c < kc; ++c)
              for (int s = 0; s < ks; ++s)
                if (back[(size_t)c * ks + s] != Cm[(size_t)c * ldc + s]) return fail("packing", (long)wi, kc);
            if (nonzero != (size_t)ks * kc) return fail("padding", (long)wi, kc);
          }
  }
  // the Gram plans: every shape, the refused split included; a grid is never empty and never beyond its partial Grams
  for (size_t m : {(size_t)1, (size_t)15, (size_t)16, (size_t)31, (size_t)1000, (size_t)1001, (size_t)1004, (size_t)100004})
    for (int ka : {1, 15, 16, 17, 48, 49, 80, 81, 96})
      for (int kb : {1, 15, 16, 17, 48, 49, 80, 81, 96})
        for (int bits = 0; bits < 16; ++bits)
          for (int num_cu : {1, 256}) {
            const mi::GramPlan p = mi::gram_plan(m, ka, kb, bits & 1, bits & 2, bits & 4, bits & 8, num_cu);
            if (p.ok != (!(bits & 2) || p.direct)) return fail("refusal", (long)m, ka);
            if (p.direct ? (p.nwaves < 4 || p.nwaves % 4 || p.nb != p.nwaves + p.tail || p.T < 1 || p.T > 5)
                         : (p.nb < 1 || p.tpw < 1 || p.tpw > 5 || p.lds == 0))
              return fail("gram plan", (long)m, ka);
            const mi::GramPairPlan q = mi::gram_pair_plan(m, ka, bits & 1, bits & 2, num_cu);
            if (q.T < 1 || q.T > 5 || q.nwaves % 4 || (q.half && !q.pair)) return fail("pair plan", (long)m, ka);
            if (mi::gram_direct_ok(m, ka, bits & 4, mi::kGramPairMinRows) && q.nwaves < 4) return fail("pair grid", (long)m, ka);
          }
  // the sweep plans around the widest plane the grid holds; D = 0 is refused without a division
  const size_t edge = (size_t)mi::kPlanSwRows * mi::kPlanMaxRows;
  for (size_t D : {(size_t)0, (size_t)1, (size_t)1024, (size_t)15876, edge - 1, edge, edge + 1, ((size_t)1 << 22) - 1})
    for (size_t nst : {(size_t)1, (size_t)12, (size_t)126, (size_t)500})
      for (int k : {1, 24, 96})
        for (int zopt : {0, 7, 5000}) {
          const mi::SweepPlan p = mi::sweep_plan(D, D * nst, k, 256, zopt);
          if (p.ok != (D >= 1 && D <= edge) || p.ok != mi::sweep_fits(D)) return fail("sweep refusal", (long)D, k);
          if (p.ok && (p.xgrid != p.tiles * p.zsegs || p.xgrid > mi::kPlanMaxRows || (size_t)p.zs * p.zsegs < nst || p.zsegs < 1))
            return fail("sweep plan", (long)D, k);
        }
  std::printf("sanitize_lobpcg_plan: ok\n");
  return 0;
}
