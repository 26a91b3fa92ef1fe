// Device pieces of the similarity alignment (ba_similarity; include/ba_hip.h, "similarity alignment").  Included
// inside the unnamed namespace of ba_similarity_kernels.hip after ba_refine_dev.h (rotation_vector_reg, RS_SWEEPS).  gfx950 only;
// built without FMA contraction like the rest.
//
// dst ~ s R src + t from the 16 sums of a set about its first row (Umeyama's closed form): the mean-free covariance K = U Sigma V'
// by the one-sided Jacobi of nearest_rotation, R = U diag(1, 1, d) V', s = trace(Sigma diag(1, 1, d)) / v_a.  Everything lives in
// the registers of ONE LANE -- a 3 x 3 Jacobi needs no LDS slab -- and every lane of a wave (a hypothesis) or of a workgroup (the
// fit of a set) runs it on the same sums and holds the same bits.  The loops over rows and columns are unrolled and the column of
// the smallest singular value is taken by selection, so that no array is indexed by a variable (an indexed private array would go
// to scratch).
#pragma once

constexpr int SM_ROW = 7;    // a row record: src (3), dst (3), used (1.0 / 0.0)
constexpr int SM_SUMS = 16;  // sum a (3), sum b (3), sum |a|^2 (1), sum b a' (9, row-major)
constexpr int SM_FIT = 13;   // a fit: s, R (9, row-major), t (3)

// the 16 terms of one row about the origin row (so, do); the caller adds them up (a lane without a row passes zeros)
__device__ __forceinline__ void similarity_terms(const double *row, const double so[3], const double dq[3], double term[SM_SUMS]) {
  const double a0 = row[0] - so[0], a1 = row[1] - so[1], a2 = row[2] - so[2];
  const double b0 = row[3] - dq[0], b1 = row[4] - dq[1], b2 = row[5] - dq[2];
  term[0] = a0, term[1] = a1, term[2] = a2;
  term[3] = b0, term[4] = b1, term[5] = b2;
  term[6] = (a0 * a0 + a1 * a1) + a2 * a2;
  term[7] = b0 * a0, term[8] = b0 * a1, term[9] = b0 * a2;
  term[10] = b1 * a0, term[11] = b1 * a1, term[12] = b1 * a2;
  term[13] = b2 * a0, term[14] = b2 * a1, term[15] = b2 * a2;
}

// one rotation of the column pair (P, Q) of W (and of V3) where the two columns are not orthogonal yet; returns 1 if it rotated
template <int P, int Q>
__device__ __forceinline__ int similarity_rotate(double W[9], double V3[9]) {
  const double al = (W[P] * W[P] + W[3 + P] * W[3 + P]) + W[6 + P] * W[6 + P];
  const double be = (W[Q] * W[Q] + W[3 + Q] * W[3 + Q]) + W[6 + Q] * W[6 + Q];
  const double ga = (W[P] * W[Q] + W[3 + P] * W[3 + Q]) + W[6 + P] * W[6 + Q];
  if (!(fabs(ga) > 1e-16 * sqrt(al * be))) return 0;  // (also ends on a NaN)
  const double ze = (be - al) / (2.0 * ga);
  const double tt = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(ze * ze + 1.0));
  const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double wp = W[3 * i + P], wq = W[3 * i + Q];
    W[3 * i + P] = cs * wp - sn * wq;
    W[3 * i + Q] = sn * wp + cs * wq;
    const double vp = V3[3 * i + P], vq = V3[3 * i + Q];
    V3[3 * i + P] = cs * vp - sn * vq;
    V3[3 * i + Q] = sn * vp + cs * vq;
  }
  return 1;
}

// The fit of the header from the 16 sums S of m rows about the origin row (so, dq): P <- s, R, t.  false: degenerate -- a sum that
// is not finite, v_a <= 0, sigma_2 <= 1e-10 sigma_1 (collinear rows), s not finite or <= 0.  (one lane)
__device__ __forceinline__ bool similarity_from_sums(const double S[SM_SUMS], double m, const double so[3], const double dq[3], int with_scale,
                                                     double P[SM_FIT]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < SM_SUMS; i++) ok = ok && isfinite(S[i]);
  if (!ok) return false;
  const double ma[3] = {S[0] / m, S[1] / m, S[2] / m}, mb[3] = {S[3] / m, S[4] / m, S[5] / m};
  const double va = S[6] - m * ((ma[0] * ma[0] + ma[1] * ma[1]) + ma[2] * ma[2]);
  if (!(va > 0.0)) return false;
  double W[9], V3[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      W[3 * i + j] = S[7 + 3 * i + j] - (m * mb[i]) * ma[j];
      V3[3 * i + j] = i == j ? 1.0 : 0.0;
    }
#pragma nounroll
  for (int sweep = 0; sweep < RS_SWEEPS; sweep++) {
    int rotated = similarity_rotate<0, 1>(W, V3);
    rotated |= similarity_rotate<0, 2>(W, V3);
    rotated |= similarity_rotate<1, 2>(W, V3);
    if (!rotated) break;
  }
  const double g0 = sqrt((W[0] * W[0] + W[3] * W[3]) + W[6] * W[6]);
  const double g1 = sqrt((W[1] * W[1] + W[4] * W[4]) + W[7] * W[7]);
  const double g2 = sqrt((W[2] * W[2] + W[5] * W[5]) + W[8] * W[8]);
  int jm = 0;
  double gm = g0;
  if (g1 < gm) jm = 1, gm = g1;
  if (g2 < gm) jm = 2, gm = g2;
  // (ja, jb, jm) is a cyclic order: det U = +1 = det V3
  const double ga = jm == 2 ? g0 : (jm == 0 ? g1 : g2), gb = jm == 2 ? g1 : (jm == 0 ? g2 : g0);
  const double s1 = fmax(ga, gb), s2 = fmin(ga, gb);
  if (!(isfinite(s1) && isfinite(s2) && isfinite(gm)) || !(s2 > 1e-10 * s1)) return false;
  double ua[3], ub[3], wm[3], um[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double w0 = W[3 * i], w1 = W[3 * i + 1], w2 = W[3 * i + 2];
    ua[i] = (jm == 2 ? w0 : (jm == 0 ? w1 : w2)) / ga;
    ub[i] = (jm == 2 ? w1 : (jm == 0 ? w2 : w0)) / gb;
    wm[i] = jm == 2 ? w2 : (jm == 0 ? w0 : w1);
  }
  um[0] = ua[1] * ub[2] - ua[2] * ub[1];
  um[1] = ua[2] * ub[0] - ua[0] * ub[2];
  um[2] = ua[0] * ub[1] - ua[1] * ub[0];
  // d = -1 iff the column so taken points against K's own: the sign was turned
  const double d = (um[0] * wm[0] + um[1] * wm[1]) + um[2] * wm[2] < 0.0 ? -1.0 : 1.0;
  double U[9];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    U[3 * i] = jm == 2 ? ua[i] : (jm == 0 ? um[i] : ub[i]);
    U[3 * i + 1] = jm == 2 ? ub[i] : (jm == 0 ? ua[i] : um[i]);
    U[3 * i + 2] = jm == 2 ? um[i] : (jm == 0 ? ub[i] : ua[i]);
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) P[1 + 3 * i + j] = (U[3 * i] * V3[3 * j] + U[3 * i + 1] * V3[3 * j + 1]) + U[3 * i + 2] * V3[3 * j + 2];
  const double s = with_scale ? ((s1 + s2) + d * gm) / va : 1.0;
  if (!isfinite(s) || !(s > 0.0)) return false;
  P[0] = s;
  const double c0 = so[0] + ma[0], c1 = so[1] + ma[1], c2 = so[2] + ma[2];
#pragma unroll
  for (int i = 0; i < 3; i++) P[10 + i] = (dq[i] + mb[i]) - s * ((P[1 + 3 * i] * c0 + P[2 + 3 * i] * c1) + P[3 + 3 * i] * c2);
  return true;
}

// |s R src + t - dst|^2 of a row record under the fit P
__device__ __forceinline__ double similarity_residual2(const double *row, const double P[SM_FIT]) {
  const double x0 = row[0], x1 = row[1], x2 = row[2];
  const double e0 = (P[0] * ((P[1] * x0 + P[2] * x1) + P[3] * x2) + P[10]) - row[3];
  const double e1 = (P[0] * ((P[4] * x0 + P[5] * x1) + P[6] * x2) + P[11]) - row[4];
  const double e2 = (P[0] * ((P[7] * x0 + P[8] * x1) + P[9] * x2) + P[12]) - row[5];
  return (e0 * e0 + e1 * e1) + e2 * e2;
}

// The inlier test of the header on a row record under the fit P: used and |s R src + t - dst|^2 <= tau^2 (a comparison with NaN
// fails).  The one test of every kernel that tests a row under a similarity.
__device__ __forceinline__ bool similarity_inlier(const double *row, const double P[SM_FIT], double tau2) {
  if (row[6] == 0.0) return false;
  return similarity_residual2(row, P) <= tau2;
}
