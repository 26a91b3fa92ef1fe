// Device pieces of the homography of a camera pair (ba_homography, ba_decompose_homography, ba_homography_pose; include/ba_hip.h,
// "homography of camera pairs").  Included inside the unnamed namespace of ba_homography_kernels.hip after ba_refine_dev.h
// and ba_consensus_dev.h, whose pieces it calls as they are: wave_all_sum, image_stats, normalised_ray, the 12 x 12 Jacobi with
// the 9 x 9 matrix in it (epipolar_trace, epipolar_matrix_entry, smallest_eigenpair<9>), the 3 x 3 Jacobi SVD (nearest_rotation,
// for its singular values) and rotation_vector_reg.  gfx950 only; built without FMA contraction like the rest.
//
// d_b x (H d_a) = 0 for the rays d = (q, -1) of a match on a plane.  On Hartley-normalised rays the three rows of that equation
// are A = [d~_b]x (x) d~_a' (3 x 9, h~ row-major), and A'A = G (x) (d~_a d~_a') with G = [d~_b]x'[d~_b]x = |d~_b|^2 I - d~_b d~_b':
// the 45 packed sums of a 9 x 9 matrix, as many as the eight-point fit takes, so the LDS of a fit is the PairScratch of that fit.
// H of a fit lives in sh.Rc[0..9) (the candidate rotations of the essential matrix have no counterpart here).
#pragma once


// the 45 terms of one match; the caller adds them up (a lane without a match passes zeros)
__device__ __forceinline__ void homography_terms(const double da[3], const double db[3], double term[EP_SUMS]) {
  const double b2 = (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
  double G[9], D[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      G[3 * i + j] = (i == j ? b2 : 0.0) - db[i] * db[j];
      D[3 * i + j] = da[i] * da[j];
    }
  int tt = 0;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j <= i; j++, tt++) term[tt] = G[3 * (i / 3) + j / 3] * D[3 * (i % 3) + j % 3];
}

// From eigenvector i1 of sh.rs.V = H~: H = T_b^-1 H~ T_a with T = [[s, 0, s c_x], [0, s, s c_y], [0, 0, 1]], its singular values by
// nearest_rotation, H / sigma_2 -> sh.Rc[0..9).  false: a singular value or an entry that is not finite, or sigma_3 <= 1e-6
// sigma_1.  (one lane)
__device__ __forceinline__ bool homography_from_eigenvector(PairScratch &sh, int i1, const double ca[2], double sa, const double cb[2],
                                                            double sb) {
  ResectScratch &rs = sh.rs;
  for (int i = 0; i < 3; i++) {  // G = H~ T_a
    const double h0 = rs.V[(3 * i) * 12 + i1], h1 = rs.V[(3 * i + 1) * 12 + i1], h2 = rs.V[(3 * i + 2) * 12 + i1];
    sh.Rc[3 * i] = h0 * sa, sh.Rc[3 * i + 1] = h1 * sa, sh.Rc[3 * i + 2] = h2 + sa * (h0 * ca[0] + h1 * ca[1]);
  }
  for (int j = 0; j < 3; j++) {  // H = T_b^-1 G
    const double g0 = sh.Rc[j], g1 = sh.Rc[3 + j], g2 = sh.Rc[6 + j];
    sh.Rc[j] = g0 / sb - cb[0] * g2, sh.Rc[3 + j] = g1 / sb - cb[1] * g2;
  }
  for (int e = 0; e < 9; e++) rs.W[e] = sh.Rc[e];
  nearest_rotation(rs);
  const double a = rs.sg[0], b = rs.sg[1], c = rs.sg[2];
  const double s1 = fmax(a, fmax(b, c)), s3 = fmin(a, fmin(b, c)), s2 = fmax(fmin(a, b), fmin(fmax(a, b), c));
  if (!(isfinite(s1) && isfinite(s2) && isfinite(s3)) || !(s3 > 1e-6 * s1)) return false;
  bool ok = true;
  for (int e = 0; e < 9; e++) {
    sh.Rc[e] = sh.Rc[e] / s2;
    ok = ok && isfinite(sh.Rc[e]);
  }
  return ok;
}

// The fit from the 45 sums sh.S (all finite, a Sync behind their writes) of rays normalised with (c, s) per image: M, its smallest
// eigenvector, H at sigma_2 = 1 -> sh.Rc[0..9) under the eigenvector's sign (lane 0; a Sync behind it).  false: degenerate.
// Called by `lanes` lanes (t: 0 .. lanes - 1) that Sync orders, as jacobi12; the result is uniform over them.
template <void (*Sync)()>
__device__ __forceinline__ bool homography_from_sums(PairScratch &sh, int t, int lanes, const double ca[2], double sa, const double cb[2],
                                                     double sb) {
  const double tr = epipolar_trace(sh.S);
  for (int e = t; e < 144; e += lanes) sh.rs.M[e] = epipolar_matrix_entry(sh.S, tr, e);
  jacobi12<Sync>(sh.rs.M, sh.rs.V, t, lanes);
  int i1;
  if (!smallest_eigenpair<9>(sh.rs.M, i1)) return false;
  if (t == 0) sh.ok = homography_from_eigenvector(sh, i1, ca, sa, cb, sb) ? 1 : 0;
  Sync();
  return sh.ok != 0;
}

// d_b' H d_a of a match, d = (q, -1): positive for a point in front of both cameras under the right sign of H
__device__ __forceinline__ double homography_side(const double *H, double qax, double qay, double qbx, double qby) {
  const double m0 = (H[0] * qax + H[1] * qay) - H[2], m1 = (H[3] * qax + H[4] * qay) - H[5], m2 = (H[6] * qax + H[7] * qay) - H[8];
  return (qbx * m0 + qby * m1) - m2;
}

// the sign of the fit: H is negated iff fewer than half of the n matches of the set have d_b' H d_a > 0 (pos of them do) or, at
// exactly half, det H < 0 -- the eigenvector's own sign is arbitrary and must not decide
__device__ __forceinline__ void homography_sign(PairScratch &sh, int pos, int n) {
  const double *H = sh.Rc;
  const double det = (H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6])) + H[2] * (H[3] * H[7] - H[4] * H[6]);
  if (2 * pos < n || (2 * pos == n && det < 0.0))
    for (int e = 0; e < 9; e++) sh.Rc[e] = -sh.Rc[e];
}

// what a lane tests matches under: H and its adjugate (the inverse up to det H: no division, and the ratios need no scale)
struct HomMap {
  double H[9], A[9];
};
__device__ __forceinline__ void homography_map_of(const double *H, HomMap &P) {
#pragma unroll
  for (int e = 0; e < 9; e++) P.H[e] = H[e];
  P.A[0] = H[4] * H[8] - H[5] * H[7], P.A[1] = H[2] * H[7] - H[1] * H[8], P.A[2] = H[1] * H[5] - H[2] * H[4];
  P.A[3] = H[5] * H[6] - H[3] * H[8], P.A[4] = H[0] * H[8] - H[2] * H[6], P.A[5] = H[2] * H[3] - H[0] * H[5];
  P.A[6] = H[3] * H[7] - H[4] * H[6], P.A[7] = H[1] * H[6] - H[0] * H[7], P.A[8] = H[0] * H[4] - H[1] * H[3];
}

// The inlier test of the header on a ray record (q_a, q_b, used) under H: used, m = H d_a and m' = adj(H) d_b with a negative third
// entry, and both transfer errors in pixels^2 within tau^2 (a comparison with NaN fails).  The one test of every kernel that
// tests a match under a homography.
__device__ __forceinline__ bool homography_inlier(const double *ray, const HomMap &P, double fa, double fb, double tau2) {
  if (ray[4] == 0.0) return false;
  const double qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
  const double m0 = (P.H[0] * qax + P.H[1] * qay) - P.H[2], m1 = (P.H[3] * qax + P.H[4] * qay) - P.H[5];
  const double m2 = (P.H[6] * qax + P.H[7] * qay) - P.H[8];
  if (!(m2 < 0.0)) return false;
  const double n0 = (P.A[0] * qbx + P.A[1] * qby) - P.A[2], n1 = (P.A[3] * qbx + P.A[4] * qby) - P.A[5];
  const double n2 = (P.A[6] * qbx + P.A[7] * qby) - P.A[8];
  if (!(n2 < 0.0)) return false;
  const double bx = qbx + m0 / m2, by = qby + m1 / m2, ax = qax + n0 / n2, ay = qay + n1 / n2;
  const double eb = (fb * fb) * (bx * bx + by * by), ea = (fa * fa) * (ax * ax + ay * ay);
  return eb <= tau2 && ea <= tau2;
}

// ---- the decomposition (Ma, Soatto, Kosecka, Sastry, An Invitation to 3-D Vision, Alg. 5.2) in the registers of ONE LANE -----------
// Every loop over the columns is unrolled, so that no array is indexed by a variable (an indexed private array would go to
// scratch): the reason rotation_vector_reg exists beside rotation_vector.

// one rotation of the one-sided Jacobi SVD on the columns (wp, wq) of W = H V and (vp, vq) of V; false: they are orthogonal
__device__ __forceinline__ bool svd3_rotate(double wp[3], double wq[3], double vp[3], double vq[3]) {
  const double al = (wp[0] * wp[0] + wp[1] * wp[1]) + wp[2] * wp[2], be = (wq[0] * wq[0] + wq[1] * wq[1]) + wq[2] * wq[2];
  const double ga = (wp[0] * wq[0] + wp[1] * wq[1]) + wp[2] * wq[2];
  if (!(fabs(ga) > 1e-16 * sqrt(al * be))) return false;
  const double ze = (be - al) / (2.0 * ga);
  const double tt = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(ze * ze + 1.0));
  const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double a = wp[i], b = wq[i], c = vp[i], d = vq[i];
    wp[i] = cs * a - sn * b, wq[i] = sn * a + cs * b;
    vp[i] = cs * c - sn * d, vq[i] = sn * c + cs * d;
  }
  return true;
}

__device__ __forceinline__ void svd3_swap(double &sa, double &sb, double wa[3], double wb[3], double va[3], double vb[3]) {
  if (!(sa < sb)) return;
  double x = sa;
  sa = sb, sb = x;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    x = wa[i], wa[i] = wb[i], wb[i] = x;
    x = va[i], va[i] = vb[i], vb[i] = x;
  }
}

// v (and w = H v with it) signed so that v's entry of the largest magnitude is positive, ties to the lowest index
__device__ __forceinline__ void svd3_sign(double v[3], double w[3]) {
  double big = v[0];
  if (fabs(v[1]) > fabs(big)) big = v[1];
  if (fabs(v[2]) > fabs(big)) big = v[2];
  if (big < 0.0) {
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = -v[i], w[i] = -w[i];
  }
}

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void mat3_vec(const double H[9], const double v[3], double out[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = (H[3 * i] * v[0] + H[3 * i + 1] * v[1]) + H[3 * i + 2] * v[2];
}

// slot s of the outputs <- (R, t, n) and slot s + 1 <- (R, -t, -n)
__device__ __forceinline__ void homography_store_pair(double *R, double *t, double *nrm, int s, const double Rm[9], const double tv[3],
                                                      const double nv[3]) {
#pragma unroll
  for (int e = 0; e < 9; e++) R[9 * s + e] = Rm[e], R[9 * (s + 1) + e] = Rm[e];
#pragma unroll
  for (int e = 0; e < 3; e++) {
    t[3 * s + e] = tv[e], t[3 * (s + 1) + e] = -tv[e];
    nrm[3 * s + e] = nv[e], nrm[3 * (s + 1) + e] = -nv[e];
  }
}

// The decomposition of the header: H (row-major, its sign as given) -> R (4 x 9), t (4 x 3, in units of the plane distance), nrm
// (4 x 3), the unused slots NaN; parallax = sigma_1 - sigma_3 at sigma_2 = 1 (NaN with 0 solutions).  Returns 0 (an entry or a
// singular value that is not finite, sigma_2 = 0), 1 (sigma_1^2 - sigma_3^2 <= 1e-12: a rotation, t = 0, n = 0) or 4.  The
// outputs may lie in LDS or in global memory.  (one lane)
__device__ __forceinline__ int homography_decompose(const double Hin[9], double *R, double *t, double *nrm, double &parallax) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int e = 0; e < 36; e++) R[e] = nan;
  for (int e = 0; e < 12; e++) t[e] = nan, nrm[e] = nan;
  parallax = nan;
  bool fin = true;
#pragma unroll
  for (int e = 0; e < 9; e++) fin = fin && isfinite(Hin[e]);
  if (!fin) return 0;
  double w1[3] = {Hin[0], Hin[3], Hin[6]}, w2[3] = {Hin[1], Hin[4], Hin[7]}, w3[3] = {Hin[2], Hin[5], Hin[8]};
  double v1[3] = {1.0, 0.0, 0.0}, v2[3] = {0.0, 1.0, 0.0}, v3[3] = {0.0, 0.0, 1.0};
#pragma nounroll
  for (int sweep = 0; sweep < RS_SWEEPS; sweep++) {
    const bool r01 = svd3_rotate(w1, w2, v1, v2);
    const bool r02 = svd3_rotate(w1, w3, v1, v3);
    const bool r12 = svd3_rotate(w2, w3, v2, v3);
    if (!(r01 || r02 || r12)) break;
  }
  double s1 = sqrt((w1[0] * w1[0] + w1[1] * w1[1]) + w1[2] * w1[2]), s2 = sqrt((w2[0] * w2[0] + w2[1] * w2[1]) + w2[2] * w2[2]);
  double s3 = sqrt((w3[0] * w3[0] + w3[1] * w3[1]) + w3[2] * w3[2]);
  svd3_swap(s1, s2, w1, w2, v1, v2);
  svd3_swap(s2, s3, w2, w3, v2, v3);
  svd3_swap(s1, s2, w1, w2, v1, v2);
  if (!(isfinite(s1) && isfinite(s3)) || !(s2 > 0.0)) return 0;
  svd3_sign(v1, w1);
  svd3_sign(v3, w3);
  cross3(v3, v1, v2);  // V = [v1, v2, v3] is a proper rotation
  double H[9];
#pragma unroll
  for (int e = 0; e < 9; e++) H[e] = Hin[e] / s2;
  const double g1 = s1 / s2, g3 = s3 / s2;
  parallax = g1 - g3;
  const double dd = g1 * g1 - g3 * g3;
  double Hv2[3];
  mat3_vec(H, v2, Hv2);
  if (!(dd > 1e-12)) {  // a rotation: U V' with U = [H v1 / sigma_1, H v2, their cross product]
    double u1[3] = {w1[0] / s1, w1[1] / s1, w1[2] / s1}, u3[3];
    cross3(u1, Hv2, u3);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) R[3 * i + j] = (u1[i] * v1[j] + Hv2[i] * v2[j]) + u3[i] * v3[j];
#pragma unroll
    for (int e = 0; e < 3; e++) t[e] = 0.0, nrm[e] = 0.0;
    return 1;
  }
  const double ca = sqrt(fmax(1.0 - g3 * g3, 0.0)), cb = sqrt(fmax(g1 * g1 - 1.0, 0.0)), cd = sqrt(dd);
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const double sg = s == 0 ? 1.0 : -1.0;
    double u[3], Hu[3], nv[3], c[3], Rm[9], tv[3];
#pragma unroll
    for (int i = 0; i < 3; i++) u[i] = (ca * v1[i] + sg * (cb * v3[i])) / cd;
    mat3_vec(H, u, Hu);
    cross3(v2, u, nv);
    cross3(Hv2, Hu, c);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Rm[3 * i + j] = (Hv2[i] * v2[j] + Hu[i] * u[j]) + c[i] * nv[j];
#pragma unroll
    for (int i = 0; i < 3; i++)
      tv[i] = ((H[3 * i] - Rm[3 * i]) * nv[0] + (H[3 * i + 1] - Rm[3 * i + 1]) * nv[1]) + (H[3 * i + 2] - Rm[3 * i + 2]) * nv[2];
    homography_store_pair(R, t, nrm, 2 * s, Rm, tv, nv);
  }
  return 4;
}
