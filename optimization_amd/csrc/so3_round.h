// so3_round.h -- the rotation nearest to a 3x3 block M in the Frobenius norm, U diag(1, 1, det(U V')) V' for M = U Sigma V',
// as straight-line fp64 code for one lane (so3.hip: k_so3_round) that a host compiler takes too.
//
// Method: one-sided (Hestenes) Jacobi.  A = M J_1 J_2 ..., V = J_1 J_2 ... with plane rotations J chosen to make two
// columns of A orthogonal; after kSo3RoundSweeps cyclic sweeps over the three pairs A = U Sigma column by column (the
// iteration converges quadratically: a 3x3 block is at rounding level after four sweeps, the last two cost nothing that
// matters next to the loads).  Every rotation is computed and applied unconditionally -- a pair that is orthogonal
// already gets t = 0 by a select -- so the lanes of a wave run the same instructions whatever their blocks.
// The rotation is then built WITHOUT the determinant: with p, q the columns of the two largest singular values,
//     R = u_p v_p' + u_q v_q' + (u_p x u_q) (v_p x v_q)'
// is the rotation that takes v_p to u_p and v_q to u_q, which is what U diag(1, 1, d) V' does for either sign of d: a
// block with det < 0 has its SMALLEST singular direction flipped by construction, a singular block (sigma_3 = 0) needs no
// third left vector, and no sign is decided by a rounded determinant.  u_q and v_q are re-orthogonalised against u_p and
// v_p once, so R' R - I is a few roundings whatever the sweeps left.
// The block is scaled by its largest entry first (the polar factor does not change): no square over- or underflows.
// Reported beside R: sep = (sigma_2 + d sigma_3) / sigma_1 with d = sign det(A) = sign det(M) (V is a product of
// rotations), the quantity the conditioning of the projection goes with; degenerate: a block with a non-finite entry,
// the zero block, or one whose projection is not finite (rank one: the nearest rotation is not unique) -- R = I.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define MI_SO3_HD __host__ __device__ __forceinline__
#else
#define MI_SO3_HD inline
#endif

namespace mi {

constexpr int kSo3RoundSweeps = 6;

// det M (row-major), contraction off: the counting pass and the rounding pass must see the same sign for the same bits
MI_SO3_HD double so3_det3(const double *M) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c0 = M[4] * M[8] - M[5] * M[7], c1 = M[3] * M[8] - M[5] * M[6], c2 = M[3] * M[7] - M[4] * M[6];
  return (M[0] * c0 - M[1] * c1) + M[2] * c2;
}

// columns (ap, aq) <- (ap, aq) J, (vp, vq) <- (vp, vq) J with J the plane rotation after which ap . aq = 0
MI_SO3_HD void so3_jacobi_pair(double *ap, double *aq, double *vp, double *vq) {
  const double alpha = ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2];
  const double beta = aq[0] * aq[0] + aq[1] * aq[1] + aq[2] * aq[2];
  const double gamma = ap[0] * aq[0] + ap[1] * aq[1] + ap[2] * aq[2];
  const double zeta = (beta - alpha) / (2 * gamma);
  // the smaller root of t^2 + 2 zeta t - 1 = 0; gamma = 0 (zeta infinite or 0 / 0) and an overflowing zeta^2 give t = 0
  double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1 + zeta * zeta));
  t = (gamma != 0 && t == t) ? t : 0.0;
  const double c = 1 / sqrt(1 + t * t), s = c * t;
  for (int r = 0; r < 3; ++r) {
    const double x = ap[r], y = aq[r], vx = vp[r], vy = vq[r];
    ap[r] = c * x - s * y;
    aq[r] = s * x + c * y;
    vp[r] = c * vx - s * vy;
    vq[r] = s * vx + c * vy;
  }
}

MI_SO3_HD void so3_cross(const double *a, const double *b, double *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// b <- the unit vector along b - (a . b) a, a a unit vector
MI_SO3_HD void so3_orthonormal_to(const double *a, double *b) {
  const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double b0 = b[0] - ab * a[0], b1 = b[1] - ab * a[1], b2 = b[2] - ab * a[2];
  const double n = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
  b[0] = b0 / n; b[1] = b1 / n; b[2] = b2 / n;
}

// M, R: row-major 3x3 (R may be M).  sep: see above (0 for a degenerate block); d: +1 / -1, the sign used in sep.
MI_SO3_HD void so3_nearest_rotation(const double *M, double *R, double &sep, double &d, bool &degenerate) {
  double big = 0, fin = 0;
  for (int c = 0; c < 9; ++c) {
    big = fmax(big, fabs(M[c]));
    fin += M[c] * 0.0;  // NaN as soon as one entry is not finite
  }
  const bool bad = !(fin == 0.0) || !(big > 0);
  const double scale = bad ? 1.0 : big;
  double a[3][3], v[3][3];  // a[k]: column k of A; v[k]: column k of V
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) {
      a[k][r] = bad ? (k == r ? 1.0 : 0.0) : M[3 * r + k] / scale;
      v[k][r] = k == r ? 1.0 : 0.0;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int sweep = 0; sweep < kSo3RoundSweeps; ++sweep) {
    so3_jacobi_pair(a[0], a[1], v[0], v[1]);
    so3_jacobi_pair(a[0], a[2], v[0], v[2]);
    so3_jacobi_pair(a[1], a[2], v[1], v[2]);
  }
  double n[3], a12[3];
  for (int k = 0; k < 3; ++k) n[k] = a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2];
  so3_cross(a[1], a[2], a12);
  const double detA = a[0][0] * a12[0] + a[0][1] * a12[1] + a[0][2] * a12[2];
  // m: the column of the smallest singular value; p: of the largest; q: the third (selects, no indexed registers)
  const bool m0 = n[0] <= n[1] && n[0] <= n[2], m1 = !m0 && n[1] <= n[2];
  const double nA = m0 ? n[1] : m1 ? n[2] : n[0], nB = m0 ? n[2] : m1 ? n[0] : n[1], nm = m0 ? n[0] : m1 ? n[1] : n[2];
  const bool sw = nB > nA;
  double up[3], uq[3], vp[3], vq[3], u3[3], v3[3];
  for (int r = 0; r < 3; ++r) {
    const double aA = m0 ? a[1][r] : m1 ? a[2][r] : a[0][r], aB = m0 ? a[2][r] : m1 ? a[0][r] : a[1][r];
    const double vA = m0 ? v[1][r] : m1 ? v[2][r] : v[0][r], vB = m0 ? v[2][r] : m1 ? v[0][r] : v[1][r];
    up[r] = sw ? aB : aA; uq[r] = sw ? aA : aB;
    vp[r] = sw ? vB : vA; vq[r] = sw ? vA : vB;
  }
  const double np = sw ? nB : nA, nq = sw ? nA : nB;
  const double s1 = sqrt(np), s2 = sqrt(nq), s3 = sqrt(nm);
  const double nv = sqrt(vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2]);
  for (int r = 0; r < 3; ++r) {
    up[r] /= s1;
    vp[r] /= nv;
  }
  so3_orthonormal_to(up, uq);
  so3_orthonormal_to(vp, vq);
  so3_cross(up, uq, u3);
  so3_cross(vp, vq, v3);
  double out[9], chk = 0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      out[3 * r + c] = up[r] * vp[c] + uq[r] * vq[c] + u3[r] * v3[c];
      chk += out[3 * r + c] * 0.0;
    }
  degenerate = bad || !(chk == 0.0);
  d = detA < 0 ? -1.0 : 1.0;
  sep = degenerate ? 0.0 : (s2 + d * s3) / s1;
  for (int c = 0; c < 9; ++c) R[c] = degenerate ? (c % 4 == 0 ? 1.0 : 0.0) : out[c];
}

}  // namespace mi
