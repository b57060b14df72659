// stiefel_tall.h -- host interface of the "tall rows" kernel family (stiefel_tall.hip): Stiefel St(n,p) fields whose
// rows hold 9 ... 16 doubles, p a run-time argument, the p x p products on the fp64 matrix pipe.  The entry points of
// stiefel.hip and sparse.hip route p > kMaxP here; everything that reads kMaxP keeps its meaning.
#pragma once
#include "mi_internal.h"

#include <algorithm>

namespace mi {

constexpr int kMaxPTall = 16;   // widest row of the tall family: one 16-column matrix-pipe tile
constexpr int kTallTile = 256;  // components of a Gram partial row: the whole 16 x 16 tile, entry (a, b) at a * 16 + b
// Gram partial rows live in ctx->partials2, ROW-major (row r at r * kTallTile): kTallRows producer rows and, behind
// them, the one row the reduce kernel leaves -- (kTallRows + 1) * kTallTile = kMaxComps * kMaxRows doubles exactly.
constexpr int kTallRows = 255;
static_assert((kTallRows + 1) * kTallTile <= kMaxComps * kMaxRows, "the tall family's partial rows fit the context's buffer");

inline bool tall_p(int p) { return p > kMaxP && p <= kMaxPTall; }
// workgroups of a tall kernel over `units` units of work: one partial row each
inline int tall_grid(const mi_ctx *ctx, size_t units) {
  return (int)std::max<size_t>(1, std::min<size_t>(units, std::min<size_t>(kTallRows, (size_t)ctx->max_grid)));
}

// what the family does not do: several ranks, the slot path, row shards, fields of 4 GiB or more (A may be null)
int tall_check(const mi_ctx *ctx, const mi_csr *A, size_t n, int p);
// W = A V
int tall_spmm(mi_ctx *ctx, const mi_csr *A, int p, const double *V, double *W);
// Z = A V - V S (S nullable) and the partial rows of sym(X'Z); *count = rows left
int tall_spmm_gram(mi_ctx *ctx, const mi_csr *A, int p, const CgState *st, const double *V, const double *X,
                   const double *S, double *Z, int *count);
// Gram rows of two fields.  variant 0: X'Z; 1: out = X + Z, out'out; 2: out = dinv_rows .* Z, X'out
int tall_gram(mi_ctx *ctx, size_t n, int p, int variant, bool sym, const double *X, const double *Z, const double *dinv,
              double *out, int *count);
// the rows summed into the reduced row by one workgroup (same order of summation as a consumer's prologue)
int tall_reduce(mi_ctx *ctx, int count);
inline const double *tall_reduced_row(const mi_ctx *ctx) { return ctx->partials2 + (size_t)kTallRows * kTallTile; }
// out = Z - X M, M the sum of the `count` Gram rows (count = 0: the reduced row is there already); dots: the partial
// rows of <Vin,out>, <out,out>, <Vin,Vin> in ctx->partials components 0, 1, 2; M_out (nullable): M, p x p
int tall_finish(mi_ctx *ctx, size_t n, int p, const CgState *st, const double *X, const double *Z, const double *Vin,
                int count, double *M_out, double *out, bool dots, int *nparts);
// Y <- Y (Y'Y)^-1/2 from the `count` Gram rows
int tall_polar(mi_ctx *ctx, size_t n, int p, double *Y, int count);

}  // namespace mi
