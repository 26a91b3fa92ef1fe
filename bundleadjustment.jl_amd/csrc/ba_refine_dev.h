// Device pieces shared by the block refinements and the relative pose (ba_point_kernels.hip, ba_camera_kernels.hip,
// ba_ransac_kernels.hip, ba_pair_kernels.hip).  Included inside the including file's unnamed namespace; gfx950 only.  These files are built without FMA contraction:
// the operand order and the parentheses here are those of the model's device functions and must stay.
//
// The linear resection is written once, further down: k_resect_cameras (one workgroup per camera) and
// the hypotheses of k_ransac_hypotheses (one wave per hypothesis) gather and reduce their 4 + 40 sums in their own way and
// share every step after that -- the same functions, so the same bits from the same sums.
//
// Two pieces are alike in several places and stay written out at their sites, because as shared functions they change the
// instructions of kernels that are to keep them (tools/compare_code_objects.py against the build before): the load of an
// observation's information factors with its "Lambda == 0" test (load_obs of the point kernels; observation_sums of
// k_refine_cameras; obs_used here) and the undistortion loop of point_triangulate, a copy of undistort below (with a call
// of undistort in its place the disassembly of k_refine_points differs).
#pragma once

__device__ __forceinline__ double wave_all_sum(double v) {  // every lane receives the same bits (a + b == b + a)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// z1 <- P1.z = (R X + t).z of the cam_pre row P and the point X, as jac_block forms it
__device__ __forceinline__ void p1_z(const double P[12], const double X[3], double &z1) {
  const double kx = P[0], ky = P[1], kz = P[2], s = P[9], c = P[10];
  const double d = kx * X[0] + ky * X[1] + kz * X[2];
  z1 = ((c * X[2] + s * (kx * X[1] - ky * X[0])) + ((1 - c) * d) * kz) + P[5];
}

// fixed-point iterations of the undistortion q <- u / (1 + k1 |q|^2 + k2 |q|^4), u = pt2d / f (triangulation and resection)
constexpr int UNDIST_ITERS = 8;

__device__ __forceinline__ void undistort(double ux, double uy, double k1, double k2, double &qx, double &qy) {
  qx = ux, qy = uy;
#pragma unroll
  for (int it = 0; it < UNDIST_ITERS; it++) {
    const double n2 = qx * qx + qy * qy;
    const double den = 1.0 + k1 * n2 + k2 * (n2 * n2);
    qx = ux / den;
    qy = uy / den;
  }
}

// an observation with Lambda == 0 is dropped (info: l00 l10 l11 per observation, or null)
__device__ __forceinline__ bool obs_used(const double *info, int o) {
  if (!info) return true;
  const double *l = info + 3 * (int64_t)o;
  return !(l[0] == 0.0 && l[1] == 0.0 && l[2] == 0.0);
}

// orders the LDS accesses of the wave's lanes before it against those after it
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_all_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- the linear resection: the pose of a camera from 2D-3D correspondences ---------------------------------------
// With P = R X + t the BAL projection gives q = -P.xy / P.z for the undistorted measurement q: P.x + q_x P.z = 0 and
// P.y + q_y P.z = 0, two homogeneous linear equations in the 12 entries of [R | t].  On Hartley-normalised points X~ = s (X - m),
// h = (X~, 1), the 12 x 12 normal matrix is M = [[S0, 0, Sx], [0, S0, Sy], [Sx, Sy, Sq]] with the 4 x 4 moments S0 = sum h h',
// Sx = sum q_x h h', Sy = sum q_y h h', Sq = sum |q|^2 h h'.  The eigenvector of M's smallest eigenvalue (cyclic Jacobi, M and the
// rotations in LDS) is gamma [R / s | R m + t].  A caller gathers its observations about a provisional origin, reduces the sums
// of d = X - origin and |d|^2 (hartley_stats), then the 40 moment sums (moment_terms), and runs the steps below in their order.
constexpr int RS_SUMS = 40;         // [S0 | Sx | Sy | Sq], each packed lower row-major (10)
constexpr int RS_MIN_OBS = 6;       // 12 unknowns up to scale, two equations per observation
constexpr int RS_SWEEPS = 30;       // cap of the Jacobi sweeps (12 x 12 and 3 x 3)
constexpr unsigned POSE_MASK = 0x3Fu;  // the pose components in a camera's mask of held components: any of them, no resection

// the LDS of one resection: one per workgroup in k_resect_cameras, one per wave in k_ransac_hypotheses
struct ResectScratch {
  double S[RS_SUMS];          // the moment sums on their way into M (the fill indexes LDS, not registers)
  double M[144], V[144];      // the normal matrix (its diagonal ends as the eigenvalues) and the accumulated rotations
  double W[9], V3[9], sg[3];  // the 3 x 3 block A and its one-sided Jacobi SVD: W -> U Sigma, V3, the singular values
  double U[9], R[9], r[3], tr[3];  // r: the rotation vector; tr: b, then the translation
  double f;                   // focal mode: the estimate f^ = a phi
  int ok;
};

// The mean dm of d and sc = 1 / (the RMS distance from it) from n, sum d and sum |d|^2; false: the points coincide or a sum
// is not finite
__device__ __forceinline__ bool hartley_stats(double n, const double sd[3], double sd2, double dm[3], double &sc) {
  dm[0] = sd[0] / n, dm[1] = sd[1] / n, dm[2] = sd[2] / n;
  const double var = sd2 / n - ((dm[0] * dm[0] + dm[1] * dm[1]) + dm[2] * dm[2]);
  if (!(var > 0.0) || !isfinite(var)) return false;
  sc = 1.0 / sqrt(var);
  return true;
}

// h = (X~, 1) of the point X
__device__ __forceinline__ void normalised_point(const double X[3], const double org[3], const double dm[3], double sc, double h[4]) {
  h[0] = sc * ((X[0] - org[0]) - dm[0]), h[1] = sc * ((X[1] - org[1]) - dm[1]), h[2] = sc * ((X[2] - org[2]) - dm[2]), h[3] = 1.0;
}

// the 40 terms of one observation; the caller adds them up (k_resect_cameras) or takes them as they are (one draw per lane)
__device__ __forceinline__ void moment_terms(const double h[4], double qx, double qy, double term[RS_SUMS]) {
  const double q2 = qx * qx + qy * qy;
  int tt = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j <= i; j++, tt++) {
      const double hh = h[i] * h[j];
      term[tt] = hh;
      term[10 + tt] = qx * hh;
      term[20 + tt] = qy * hh;
      term[30 + tt] = q2 * hh;
    }
}

// element e (row-major) of M from the packed sums S
__device__ __forceinline__ double normal_matrix_entry(const double *S, int e) {
  const int row = e / 12, col = e % 12, br = row >> 2, bc = col >> 2, i = row & 3, j = col & 3;
  const int hi = i > j ? i : j, lo = i > j ? j : i, tt = hi * (hi + 1) / 2 + lo;
  if (br == bc) return br == 2 ? S[30 + tt] : S[tt];
  if (br == 2 || bc == 2) return S[10 * (1 + (br == 2 ? bc : br)) + tt];
  return 0.0;
}

// Cyclic Jacobi on the symmetric 12 x 12 matrix A (row-major, both triangles kept), V <- the product of the rotations (the
// columns end as eigenvectors, the diagonal of A as eigenvalues).  A rotation is skipped when |a_pq| <= 1e-18 sqrt(|a_pp a_qq|);
// the sweeps end with the first sweep without a rotation or at RS_SWEEPS.  Called by `lanes` lanes (lane: 0 .. lanes - 1) that
// Sync orders -- a wave with wave_sync, a workgroup with __syncthreads -- A and V in LDS, A filled by those lanes (a Sync
// comes before the first read).  Every lane reads the same three entries and takes the same decision; lanes 0..11 update element
// k of the two columns of A while lanes 16..27 update it in the two columns of V, then lanes 0..11 the two rows of A, with a Sync
// between the phases.  Every element sees the operations of a one-lane loop over k.  The two groups of the first phase run one
// piece of code on a selected base pointer: as two branches they take turns inside their wave, an LDS round trip more per
// rotation, which made k_resect_cameras 3 % slower than with the rotations updated in the second phase.
template <void (*Sync)()>
__device__ __forceinline__ void jacobi12(double *A, double *V, int lane, int lanes) {
  for (int i = lane; i < 144; i += lanes) V[i] = (i / 12 == i % 12) ? 1.0 : 0.0;
  Sync();
#pragma nounroll
  for (int sweep = 0; sweep < RS_SWEEPS; sweep++) {
    int rotated = 0;
#pragma nounroll
    for (int p = 0; p < 11; p++)
#pragma nounroll
      for (int q = p + 1; q < 12; q++) {
        const double apq = A[p * 12 + q], app = A[p * 12 + p], aqq = A[q * 12 + q];
        if (!(fabs(apq) > 1e-18 * sqrt(fabs(app * aqq)))) continue;  // (uniform; also ends on a NaN)
        rotated = 1;
        const double th = (aqq - app) / (2.0 * apq);
        const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        Sync();  // (every lane has read the three entries)
        if (lane < 12 || (lane >= 16 && lane < 28)) {  // A <- A G and V <- V G: one path, so the two do not take turns
          double *T = lane < 12 ? A : V;
          const int k = lane < 12 ? lane : lane - 16;
          const double tkp = T[k * 12 + p], tkq = T[k * 12 + q];
          T[k * 12 + p] = cs * tkp - sn * tkq;
          T[k * 12 + q] = sn * tkp + cs * tkq;
        }
        Sync();
        if (lane < 12) {  // A <- G' A with a_pq = a_qp = 0
          const double apk = A[p * 12 + lane], aqk = A[q * 12 + lane];
          A[p * 12 + lane] = lane == q ? 0.0 : cs * apk - sn * aqk;
          A[q * 12 + lane] = lane == p ? 0.0 : sn * apk + cs * aqk;
        }
        Sync();
      }
    if (!rotated) break;
  }
}

// i1 <- the index of the smallest eigenvalue on the diagonal of M; false: an eigenvalue that is not finite, or the second
// smallest is not above 1e-10 of the largest (the eigenvector is not determined).  N: the leading N of the 12 are looked at (the
// 9 x 9 matrix of the relative pose sits in the 12 x 12 with three spare diagonal entries that no rotation touches).
template <int N = 12>
__device__ __forceinline__ bool smallest_eigenpair(const double *M, int &i1) {
  i1 = 0;
  double l1 = M[0], lmax = M[0];
  for (int i = 1; i < N; i++) {
    const double l = M[13 * i];
    if (l < l1) l1 = l, i1 = i;
    lmax = fmax(lmax, l);
  }
  double l2 = lmax;
  for (int i = 0; i < N; i++)
    if (i != i1) l2 = fmin(l2, M[13 * i]);
  return isfinite(l1) && isfinite(lmax) && l2 > 1e-10 * lmax;
}

// A3 . X~ + b3 of eigenvector i1: negative for a point in front of the camera under the eigenvector's sign
__device__ __forceinline__ double front_z(const double *V, int i1, const double h[4]) {
  return ((V[8 * 12 + i1] * h[0] + V[9 * 12 + i1] * h[1]) + V[10 * 12 + i1] * h[2]) + V[11 * 12 + i1];
}

// The nearest proper rotation of the 3 x 3 matrix sh.W (row-major) -> sh.R, its singular values -> sh.sg: one-sided Jacobi
// (rotations of column pairs until they are orthogonal: W V3 = U Sigma), then R = U diag(1, 1, det(U V3')) V3' with the sign on
// the smallest singular value -- its column of U is taken as the cross product of the other two, which is that sign and
// needs no division by a singular value that may be 0.  (one lane)
__device__ __forceinline__ void nearest_rotation(ResectScratch &sh) {
  for (int i = 0; i < 9; i++) sh.V3[i] = (i / 3 == i % 3) ? 1.0 : 0.0;
#pragma nounroll
  for (int sweep = 0; sweep < RS_SWEEPS; sweep++) {
    int rotated = 0;
#pragma nounroll
    for (int p = 0; p < 2; p++)
#pragma nounroll
      for (int q = p + 1; q < 3; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < 3; i++) {
          const double wp = sh.W[3 * i + p], wq = sh.W[3 * i + q];
          al += wp * wp;
          be += wq * wq;
          ga += wp * wq;
        }
        if (!(fabs(ga) > 1e-16 * sqrt(al * be))) continue;
        rotated = 1;
        const double ze = (be - al) / (2.0 * ga);
        const double tt = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(ze * ze + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int i = 0; i < 3; i++) {
          const double wp = sh.W[3 * i + p], wq = sh.W[3 * i + q];
          sh.W[3 * i + p] = cs * wp - sn * wq;
          sh.W[3 * i + q] = sn * wp + cs * wq;
          const double vp = sh.V3[3 * i + p], vq = sh.V3[3 * i + q];
          sh.V3[3 * i + p] = cs * vp - sn * vq;
          sh.V3[3 * i + q] = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  int jm = 0;
  for (int j = 0; j < 3; j++) {
    sh.sg[j] = sqrt((sh.W[j] * sh.W[j] + sh.W[3 + j] * sh.W[3 + j]) + sh.W[6 + j] * sh.W[6 + j]);
    if (sh.sg[j] < sh.sg[jm]) jm = j;
  }
  const int ja = (jm + 1) % 3, jb = (jm + 2) % 3;  // (ja, jb, jm) is a cyclic order: det U = +1 = det V3
  for (int i = 0; i < 3; i++) {
    sh.U[3 * i + ja] = sh.W[3 * i + ja] / sh.sg[ja];
    sh.U[3 * i + jb] = sh.W[3 * i + jb] / sh.sg[jb];
  }
  for (int i = 0; i < 3; i++) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    sh.U[3 * i + jm] = sh.U[3 * i1 + ja] * sh.U[3 * i2 + jb] - sh.U[3 * i2 + ja] * sh.U[3 * i1 + jb];
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      sh.R[3 * i + j] = (sh.U[3 * i] * sh.V3[3 * j] + sh.U[3 * i + 1] * sh.V3[3 * j + 1]) + sh.U[3 * i + 2] * sh.V3[3 * j + 2];
}

// The rotation vector of sh.R -> sh.r: theta = atan2(|w| / 2, (tr R - 1) / 2), w the skew part; the axis is w / |w|, and for
// cos theta < 0 it comes from the diagonal of R + I (k_i^2 = (R_ii - cos) / (1 - cos) at the largest R_ii, the others from the
// symmetric part, the sign from w); theta < 1e-12: (1e-12, 0, 0) -- the model has no theta -> 0 branch.  (one lane)
__device__ __forceinline__ void rotation_vector(ResectScratch &sh) {
  const double *R = sh.R;
  const double w0 = R[7] - R[5], w1 = R[2] - R[6], w2 = R[3] - R[1];
  const double wn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  const double co = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double th = atan2(0.5 * wn, co);
  if (th < 1e-12) {
    sh.r[0] = 1e-12, sh.r[1] = 0.0, sh.r[2] = 0.0;
  } else if (co >= 0.0) {
    sh.r[0] = th * (w0 / wn), sh.r[1] = th * (w1 / wn), sh.r[2] = th * (w2 / wn);
  } else {
    int im = 0;
    if (R[4] > R[0]) im = 1;
    if (R[8] > R[4 * im]) im = 2;
    const double ki = sqrt((R[4 * im] - co) / (1.0 - co));
    for (int j = 0; j < 3; j++) sh.r[j] = j == im ? ki : 0.5 * (R[3 * im + j] + R[3 * j + im]) / ((1.0 - co) * ki);
    const double sgn = (sh.r[0] * w0 + sh.r[1] * w1) + sh.r[2] * w2 < 0.0 ? -1.0 : 1.0;
    const double kn = sqrt((sh.r[0] * sh.r[0] + sh.r[1] * sh.r[1]) + sh.r[2] * sh.r[2]);
    for (int j = 0; j < 3; j++) sh.r[j] = th * (sgn * sh.r[j] / kn);
  }
}

// ---- the focal mode of the linear resection: f is one more unknown ------------------------------------------------
// The BAL principal point is the origin, so on raw measurements scaled by the image scale a = sqrt(sum |m|^2 / n), u = m / a,
// the same two equations read phi P.x + u_x P.z = 0 and phi P.y + u_y P.z = 0 with phi = f / a: the same normal matrix with
// q := u, whose eigenvector is gamma [phi A1; phi A2; A3 | phi b1, phi b2, b3].  The rows of A = R / s have one norm, which
// gives phi from the three rows as found; with rows 1 and 2 divided by it the eigenvector is that of the calibrated case.
constexpr unsigned FOCAL_HELD = 0x100u, K1_HELD = 0x40u, K2_HELD = 0x80u;  // in a camera's mask of held components

// whether camera mask fm runs in focal mode under the call's flag: its f is free (a group member has the bit set)
__device__ __forceinline__ bool focal_mode(int focal, unsigned fm) { return focal && !(fm & FOCAL_HELD); }

// a from n and sum |m|^2; false: not finite or 0
__device__ __forceinline__ bool image_scale(double n, double sm2, double &a) {
  a = sqrt(sm2 / n);
  return isfinite(a) && a != 0.0;
}

// phi = sqrt((|A1|^2 + |A2|^2) / (2 |A3|^2)) of eigenvector i1 of sh.V; rows 1 and 2 of [A | b] are divided by it in place and
// f^ = a phi -> sh.f.  false: phi is not finite or not positive.  In front of pose_from_eigenvector.  (one lane)
__device__ __forceinline__ bool focal_from_eigenvector(ResectScratch &sh, int i1, double a) {
  double n2[3];
  for (int i = 0; i < 3; i++) {
    const double a0 = sh.V[(4 * i) * 12 + i1], a1 = sh.V[(4 * i + 1) * 12 + i1], a2 = sh.V[(4 * i + 2) * 12 + i1];
    n2[i] = (a0 * a0 + a1 * a1) + a2 * a2;
  }
  const double phi = sqrt((n2[0] + n2[1]) / (2.0 * n2[2]));
  if (!isfinite(phi) || !(phi > 0.0)) return false;
  for (int e = 0; e < 8; e++) sh.V[e * 12 + i1] = sh.V[e * 12 + i1] / phi;
  sh.f = a * phi;
  return true;
}

// The pose from eigenvector i1 of sh.V = gamma [R / s | R m + t] under the sign sgn, with m = org + dm and s = sc: the rotation
// vector -> sh.r, t = b / gamma - R m -> sh.tr, gamma = s mean(Sigma); false: a component that is not finite.  (one lane)
__device__ __forceinline__ bool pose_from_eigenvector(ResectScratch &sh, int i1, double sgn, double sc, const double org[3],
                                                      const double dm[3]) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) sh.W[3 * i + j] = sgn * sh.V[(4 * i + j) * 12 + i1];
    sh.tr[i] = sh.V[(4 * i + 3) * 12 + i1];  // b, until the translation takes its place
  }
  nearest_rotation(sh);
  const double gam = sc * (((sh.sg[0] + sh.sg[1]) + sh.sg[2]) / 3.0);
  bool ok = true;
  for (int i = 0; i < 3; i++) {
    const double rm = (sh.R[3 * i] * (org[0] + dm[0]) + sh.R[3 * i + 1] * (org[1] + dm[1])) + sh.R[3 * i + 2] * (org[2] + dm[2]);
    sh.tr[i] = sgn * sh.tr[i] / gam - rm;
    ok = ok && isfinite(sh.tr[i]);
  }
  rotation_vector(sh);
  return ok && isfinite(sh.r[0]) && isfinite(sh.r[1]) && isfinite(sh.r[2]);
}

// ---- the eight-point relative pose: the pose of camera b against camera a from their 2D-2D matches ----------------
// P_b = R P_a + t, |t| = 1.  The BAL camera looks down -z: the ray of an undistorted measurement q is d = (q_x, q_y, -1) and a
// point in front is P = alpha d, alpha > 0.  d_b' E d_a = 0 with E = [t]x R is linear in the 9 entries of E: on Hartley-normalised
// rays d~ = (s (q - c), -1) the 9 x 9 normal matrix is M = sum a a', a = d~_b (x) d~_a (row-major e~), and the eigenvector of its
// smallest eigenvalue is E~.  M sits in the 12 x 12 of jacobi12 with trace(M) on the three spare diagonal entries and zeros beside
// them (a rotation with a_pq = 0 is skipped: the spare entries never move).  A caller gathers its matches about the first of the
// set, reduces the 6 sums of the two images (image_stats), then the 45 sums (epipolar_terms), runs essential_from_sums and counts
// the matches in front of each candidate (pair_depths) for pair_pose_winner: k_pair_hypotheses per wave, k_pair_fit per
// workgroup -- the same functions, so the same bits from the same sums.
constexpr int EP_SUMS = 45;        // M packed lower row-major
constexpr int EP_MIN_MATCHES = 8;  // 9 unknowns up to scale, one equation per match

// the LDS of one fit: one per workgroup in k_pair_fit, one per wave in k_pair_hypotheses
struct PairScratch {
  ResectScratch rs;    // M, V (the 12 x 12), the 3 x 3 SVD of E, the winner's R and rotation vector r
  double S[EP_SUMS];   // the sums on their way into M
  double Rc[18];       // the two candidate rotations U Rz(+90) V', U Rz(-90) V'
  double tn[3], t[3];  // the unit left null direction of E; the winner's translation (+ or - tn)
  int cnt[4];          // matches of the set in front under candidate c: rotation c >> 1, sign of t: c & 1
  int ok;
};

// both focal lengths of a pair's intrinsics (k1, k2, f of a, then of b) are finite and not 0
__device__ __forceinline__ bool pair_focals_ok(const double *in) {
  return isfinite(in[2]) && in[2] != 0.0 && isfinite(in[5]) && in[5] != 0.0;
}

// The Hartley normalisation of one image from n, the sums of d = q - origin and of |d|^2: the mean dm of d and s = sqrt(2) / (the
// RMS distance from it); false: the image points coincide or a sum is not finite
__device__ __forceinline__ bool image_stats(double n, double sx, double sy, double s2, double dm[3], double &s) {
  const double sd[3] = {sx, sy, 0.0};
  double sc;
  if (!hartley_stats(n, sd, s2, dm, sc)) return false;
  s = sqrt(2.0) * sc;
  return true;
}

// d~ = (s (q - c), -1) of the image point q, c = org + dm
__device__ __forceinline__ void normalised_ray(double qx, double qy, const double org[2], const double dm[3], double s, double d[3]) {
  d[0] = s * ((qx - org[0]) - dm[0]), d[1] = s * ((qy - org[1]) - dm[1]), d[2] = -1.0;
}

// the 45 terms of one match; the caller adds them up (a lane without a match passes zeros)
__device__ __forceinline__ void epipolar_terms(const double da[3], const double db[3], double term[EP_SUMS]) {
  double a[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) a[3 * i + j] = db[i] * da[j];
  int tt = 0;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j <= i; j++, tt++) term[tt] = a[i] * a[j];
}

// trace(M) from the packed sums
__device__ __forceinline__ double epipolar_trace(const double *S) {
  double tr = 0.0;
  for (int i = 0; i < 9; i++) tr += S[i * (i + 1) / 2 + i];
  return tr;
}

// element e (row-major) of the 12 x 12 that holds M, tr = trace(M)
__device__ __forceinline__ double epipolar_matrix_entry(const double *S, double tr, int e) {
  const int row = e / 12, col = e % 12;
  if (row >= 9 || col >= 9) return row == col ? tr : 0.0;
  const int hi = row > col ? row : col, lo = row > col ? col : row;
  return S[hi * (hi + 1) / 2 + lo];
}

// From eigenvector i1 of sh.rs.V = E~: E = T_b' E~ T_a with T = [[s, 0, s c_x], [0, s, s c_y], [0, 0, 1]] (d~ = T d: the third entry of d is -1), its SVD by
// nearest_rotation (U and V3 proper rotations, the column jm of the smallest singular value by cross product), the candidate
// rotations R = U Rz(+-90) V3' with Rz in the plane of the two large singular directions -> sh.Rc, the unit left null direction
// -> sh.tn.  A zero singular value among the two large ones leaves NaN, which no match is in front of.  (one lane)
__device__ __forceinline__ void essential_candidates(PairScratch &sh, int i1, const double ca[2], double sa, const double cb[2], double sb) {
  ResectScratch &rs = sh.rs;
  for (int i = 0; i < 3; i++) {  // G = E~ T_a
    const double e0 = rs.V[(3 * i) * 12 + i1], e1 = rs.V[(3 * i + 1) * 12 + i1], e2 = rs.V[(3 * i + 2) * 12 + i1];
    rs.W[3 * i] = e0 * sa, rs.W[3 * i + 1] = e1 * sa, rs.W[3 * i + 2] = e2 + sa * (e0 * ca[0] + e1 * ca[1]);
  }
  for (int j = 0; j < 3; j++) {  // E = T_b' G
    const double g0 = rs.W[j], g1 = rs.W[3 + j], g2 = rs.W[6 + j];
    rs.W[j] = sb * g0, rs.W[3 + j] = sb * g1, rs.W[6 + j] = g2 + sb * (cb[0] * g0 + cb[1] * g1);
  }
  nearest_rotation(rs);
  int jm = 0;
  for (int j = 0; j < 3; j++)
    if (rs.sg[j] < rs.sg[jm]) jm = j;
  const int ja = (jm + 1) % 3, jb = (jm + 2) % 3;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double plane = rs.U[3 * i + jb] * rs.V3[3 * j + ja] - rs.U[3 * i + ja] * rs.V3[3 * j + jb];
      const double axis = rs.U[3 * i + jm] * rs.V3[3 * j + jm];
      sh.Rc[3 * i + j] = axis + plane;
      sh.Rc[9 + 3 * i + j] = axis - plane;
    }
  const double u0 = rs.U[jm], u1 = rs.U[3 + jm], u2 = rs.U[6 + jm];
  const double un = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
  sh.tn[0] = u0 / un, sh.tn[1] = u1 / un, sh.tn[2] = u2 / un;
}

// The second half of essential_candidates from E in sh.rs.W (row-major; overwritten) on, for the five-point solver, which
// enters with each of its solutions.  A copy: with a call of it in essential_candidates the disassembly of k_pair_fit differs
// (tools/compare_code_objects.py against the build before).  (one lane)
__device__ __forceinline__ void essential_decompose(PairScratch &sh) {
  ResectScratch &rs = sh.rs;
  nearest_rotation(rs);
  int jm = 0;
  for (int j = 0; j < 3; j++)
    if (rs.sg[j] < rs.sg[jm]) jm = j;
  const int ja = (jm + 1) % 3, jb = (jm + 2) % 3;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double plane = rs.U[3 * i + jb] * rs.V3[3 * j + ja] - rs.U[3 * i + ja] * rs.V3[3 * j + jb];
      const double axis = rs.U[3 * i + jm] * rs.V3[3 * j + jm];
      sh.Rc[3 * i + j] = axis + plane;
      sh.Rc[9 + 3 * i + j] = axis - plane;
    }
  const double u0 = rs.U[jm], u1 = rs.U[3 + jm], u2 = rs.U[6 + jm];
  const double un = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
  sh.tn[0] = u0 / un, sh.tn[1] = u1 / un, sh.tn[2] = u2 / un;
}

// The fit from the 45 sums sh.S (all finite, a Sync behind their writes) of rays normalised with (c, s) per image: M, its smallest
// eigenvector, the candidates of essential_candidates (lane 0; a Sync behind them).  false: the eigenvector is not determined.
// Called by `lanes` lanes (t: 0 .. lanes - 1) that Sync orders, as jacobi12; the result is uniform over them.
template <void (*Sync)()>
__device__ __forceinline__ bool essential_from_sums(PairScratch &sh, int t, int lanes, const double ca[2], double sa, const double cb[2],
                                                    double sb) {
  const double tr = epipolar_trace(sh.S);
  for (int e = t; e < 144; e += lanes) sh.rs.M[e] = epipolar_matrix_entry(sh.S, tr, e);
  jacobi12<Sync>(sh.rs.M, sh.rs.V, t, lanes);
  int i1;
  if (!smallest_eigenpair<9>(sh.rs.M, i1)) return false;
  if (t == 0) essential_candidates(sh, i1, ca, sa, cb, sb);
  Sync();
  return true;
}

// (alpha, beta) of alpha R d_a + t = beta d_b from its 2 x 2 normal equations, d = (q, -1); t = sgn tn
__device__ __forceinline__ void pair_depths(const double *R, const double *tn, double sgn, double qax, double qay, double qbx, double qby,
                                            double &al, double &be) {
  const double u0 = (R[0] * qax + R[1] * qay) - R[2], u1 = (R[3] * qax + R[4] * qay) - R[5], u2 = (R[6] * qax + R[7] * qay) - R[8];
  const double t0 = sgn * tn[0], t1 = sgn * tn[1], t2 = sgn * tn[2];
  const double uu = (u0 * u0 + u1 * u1) + u2 * u2, vv = (qbx * qbx + qby * qby) + 1.0;
  const double uv = (u0 * qbx + u1 * qby) - u2, ut = (u0 * t0 + u1 * t1) + u2 * t2, vt = (qbx * t0 + qby * t1) - t2;
  const double det = uu * vv - uv * uv;
  al = (uv * vt - ut * vv) / det;
  be = (uu * vt - uv * ut) / det;
}

// The winner among the four candidates from sh.cnt: the most matches in front, ties to the first; its rotation vector -> sh.rs.r,
// its translation -> sh.t.  false: no match in front of any candidate, or a component that is not finite.  (one lane)
__device__ __forceinline__ bool pair_pose_winner(PairScratch &sh) {
  int best = 0;
  for (int c = 1; c < 4; c++)
    if (sh.cnt[c] > sh.cnt[best]) best = c;
  if (sh.cnt[best] <= 0) return false;
  const double sgn = (best & 1) ? -1.0 : 1.0;
  for (int i = 0; i < 9; i++) sh.rs.R[i] = sh.Rc[9 * (best >> 1) + i];
  bool ok = true;
  for (int i = 0; i < 3; i++) {
    sh.t[i] = sgn * sh.tn[i];
    ok = ok && isfinite(sh.t[i]);
  }
  rotation_vector(sh.rs);
  return ok && isfinite(sh.rs.r[0]) && isfinite(sh.rs.r[1]) && isfinite(sh.rs.r[2]);
}

// what a lane scores matches under: R of the rotation vector r (Rodrigues, no small-angle branch: rotation_vector never returns
// 0), t, and the clean E = [t]x R rebuilt from them
struct PairPose {
  double R[9], t[3], E[9];
};
__device__ __forceinline__ void pair_pose_of(const double *r, const double *t, PairPose &P) {
  const double th = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  const double kx = r[0] / th, ky = r[1] / th, kz = r[2] / th;
  const double c = cos(th), s = sin(th), v = 1.0 - c;
  P.R[0] = c + v * kx * kx, P.R[1] = v * kx * ky - s * kz, P.R[2] = v * kx * kz + s * ky;
  P.R[3] = v * ky * kx + s * kz, P.R[4] = c + v * ky * ky, P.R[5] = v * ky * kz - s * kx;
  P.R[6] = v * kz * kx - s * ky, P.R[7] = v * kz * ky + s * kx, P.R[8] = c + v * kz * kz;
  P.t[0] = t[0], P.t[1] = t[1], P.t[2] = t[2];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    P.E[j] = t[1] * P.R[6 + j] - t[2] * P.R[3 + j];
    P.E[3 + j] = t[2] * P.R[j] - t[0] * P.R[6 + j];
    P.E[6 + j] = t[0] * P.R[3 + j] - t[1] * P.R[j];
  }
}

// The inlier test of the header on a ray record (q_a, q_b, used) under P: used, alpha > 0, beta > 0 and the Sampson distance in
// pixels^2 within tau^2 (a comparison with NaN fails).  The one test of every kernel that tests a match.
__device__ __forceinline__ bool pair_inlier(const double *ray, const PairPose &P, double fa, double fb, double tau2) {
  if (ray[4] == 0.0) return false;
  const double qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
  double al, be;
  pair_depths(P.R, P.t, 1.0, qax, qay, qbx, qby, al, be);
  if (!(al > 0.0 && be > 0.0)) return false;
  const double l0 = (P.E[0] * qax + P.E[1] * qay) - P.E[2], l1 = (P.E[3] * qax + P.E[4] * qay) - P.E[5];
  const double l2 = (P.E[6] * qax + P.E[7] * qay) - P.E[8];
  const double m0 = (P.E[0] * qbx + P.E[3] * qby) - P.E[6], m1 = (P.E[1] * qbx + P.E[4] * qby) - P.E[7];
  const double num = (qbx * l0 + qby * l1) - l2;
  const double den = (l0 * l0 + l1 * l1) / (fb * fb) + (m0 * m0 + m1 * m1) / (fa * fa);
  return num * num / den <= tau2;
}

// ---- the five-point relative pose: the essential matrices through five matches -----------------------------------
// Rays are raw, d = (q, -1) in both images.  The 5 x 9 system a_k = d_b (x) d_a has a four-dimensional null space; its basis
// X, Y, Z, W is the eigenvectors of the four smallest eigenvalues of sum a a' (the 45 sums of epipolar_terms in jacobi12), and
// E = x X + y Y + z Z + W.  det E = 0 and 2 E E' E - tr(E E') E = 0 are ten cubics in the 20 monomials of (x, y, z), columns in
// the order x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.  Gauss-Jordan on the first ten columns
// leaves each of them as a polynomial in the last ten; (row x^2z) - z (row x^2), (row y^2z) - z (row y^2) and
// (row xyz) - z (row xy) hold no monomial of the first ten: B(z) (x, y, 1)' = 0 with a 3 x 3 matrix of polynomials of degree
// 3, 3, 4 in z.  det B(z) has degree 10; its roots come from the simultaneous iteration of Aberth and Ehrlich, one root per lane,
// and a root is real when its imaginary part is within 1e-7 of its modulus.  (x, y) is the null vector of B at the root, and
// (x, y, z) takes two Gauss-Newton steps on the ten cubics (five_polish).
constexpr int FP_POINTS = 5, FP_MAX_SOL = 10, FP_ROOT_ITERS = 100;
constexpr int FP_ROWS = 10, FP_COLS = 20, FP_BROW = 13;  // a row of B: x (4 coefficients, ascending), y (4), 1 (5)

// the LDS of one solve, beside the wave's PairScratch (whose S, M and V the null space goes through)
struct FiveScratch {
  double N[36];                 // X, Y, Z, W: 3 x 3 row-major each
  double C[FP_ROWS * FP_COLS];  // the ten cubics
  double B[3 * FP_BROW];
  double P[11];                 // det B(z), ascending
  double E[9 * FP_MAX_SOL];     // the real solutions, |E|_F = 1
};

// the variables (0: x, 1: y, 2: z, 3: the constant 1) of monomial m in the column order above, two bits each
__device__ __forceinline__ int five_monomial(int m) {
  // (a | b << 2 | c << 4) per monomial, six bits each: monomials 0..9 and 10..19
  const unsigned long long lo = 0ull | (21ull << 6) | (16ull << 12) | (20ull << 18) | (32ull << 24) | (48ull << 30) | (37ull << 36) |
                                (53ull << 42) | (36ull << 48) | (52ull << 54);
  const unsigned long long hi = 40ull | (56ull << 6) | (60ull << 12) | (41ull << 18) | (57ull << 24) | (61ull << 30) | (42ull << 36) |
                                (58ull << 42) | (62ull << 48) | (63ull << 54);
  return (int)(((m < 10 ? lo : hi) >> (6 * (m < 10 ? m : m - 10))) & 63ull);
}

// The trilinear form of constraint `row` on the 3 x 3 matrices A, B, C (LDS): row 0, the determinant with row 0 of A, row 1 of
// B and row 2 of C; rows 1..9, entry (i, j) of 2 A B' C - tr(A B') C.
__device__ __forceinline__ double five_form(int row, const double *A, const double *B, const double *C) {
  if (row == 0)
    return (A[0] * (B[4] * C[8] - B[5] * C[7]) + A[1] * (B[5] * C[6] - B[3] * C[8])) + A[2] * (B[3] * C[7] - B[4] * C[6]);
  const int i = (row - 1) / 3, j = (row - 1) % 3;
  double tr = 0.0, v = 0.0;
#pragma unroll
  for (int l = 0; l < 3; l++) {
    const double ab = (A[3 * i] * B[3 * l] + A[3 * i + 1] * B[3 * l + 1]) + A[3 * i + 2] * B[3 * l + 2];  // (A B')_il
    v += ab * C[3 * l + j];
    tr += (A[3 * l] * B[3 * l] + A[3 * l + 1] * B[3 * l + 1]) + A[3 * l + 2] * B[3 * l + 2];
  }
  return 2.0 * v - tr * C[3 * i + j];
}

// p(z) and p'(z) of the polynomial P (11 coefficients, ascending; LDS) at the complex z
__device__ __forceinline__ void five_horner(const double *P, double zr, double zi, double &pr, double &pi, double &dr, double &di) {
  pr = P[10], pi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
  for (int i = 9; i >= 0; i--) {
    const double tr = (dr * zr - di * zi) + pr, ti = (dr * zi + di * zr) + pi;
    dr = tr, di = ti;
    const double ur = (pr * zr - pi * zi) + P[i], ui = pr * zi + pi * zr;
    pr = ur, pi = ui;
  }
}

// v^e for e in 0..3 and its derivative, from v, v^2, v^3
__device__ __forceinline__ double five_power(int e, double v, double v2, double v3) { return e == 0 ? 1.0 : (e == 1 ? v : (e == 2 ? v2 : v3)); }
__device__ __forceinline__ double five_slope(int e, double v, double v2) { return e == 0 ? 0.0 : (e == 1 ? 1.0 : (e == 2 ? 2.0 * v : 3.0 * v2)); }

// Two Gauss-Newton steps on the ten cubics C (10 x 20, LDS; any row-equivalent form) in (x, y, z): a root of the degree-10
// determinant carries the conditioning of that polynomial, the cubics carry the solution's own.  A step that is not finite is
// not taken.  (one lane per root)
__device__ __forceinline__ void five_polish(const double *C, double &x, double &y, double &z) {
#pragma nounroll
  for (int it = 0; it < 2; it++) {
    const double x2 = x * x, x3 = x2 * x, y2 = y * y, y3 = y2 * y, z2 = z * z, z3 = z2 * z;
    double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
#pragma nounroll
    for (int i = 0; i < FP_ROWS; i++) {
      double f = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
#pragma nounroll
      for (int m = 0; m < FP_COLS; m++) {
        const int code = five_monomial(m), a = code & 3, b = (code >> 2) & 3, c = (code >> 4) & 3;
        const int ex = (a == 0) + (b == 0) + (c == 0), ey = (a == 1) + (b == 1) + (c == 1), ez = (a == 2) + (b == 2) + (c == 2);
        const double px = five_power(ex, x, x2, x3), py = five_power(ey, y, y2, y3), pz = five_power(ez, z, z2, z3);
        const double w = C[FP_COLS * i + m];
        f += w * (px * py * pz);
        fx += w * (five_slope(ex, x, x2) * py * pz);
        fy += w * (px * five_slope(ey, y, y2) * pz);
        fz += w * (px * py * five_slope(ez, z, z2));
      }
      axx += fx * fx, axy += fx * fy, axz += fx * fz, ayy += fy * fy, ayz += fy * fz, azz += fz * fz;
      gx += fx * f, gy += fy * f, gz += fz * f;
    }
    // (J'J) step = J'f by cofactors
    const double c00 = ayy * azz - ayz * ayz, c01 = axz * ayz - axy * azz, c02 = axy * ayz - axz * ayy;
    const double c11 = axx * azz - axz * axz, c12 = axy * axz - axx * ayz, c22 = axx * ayy - axy * axy;
    const double det = (axx * c00 + axy * c01) + axz * c02;
    const double sx = ((c00 * gx + c01 * gy) + c02 * gz) / det, sy = ((c01 * gx + c11 * gy) + c12 * gz) / det;
    const double sz = ((c02 * gx + c12 * gy) + c22 * gz) / det;
    if (isfinite(sx) && isfinite(sy) && isfinite(sz)) x -= sx, y -= sy, z -= sz;
  }
}

// The essential matrices through the wave's five matches: a lane with take holds one match as the rays da, db = (q, -1), every
// other lane passes zeros.  Returns the number of real solutions (0..10; 0 also for sums that are not finite, a null space that
// is not four-dimensional -- lambda_5 <= 1e-12 lambda_9 -- and a pivot that is 0 or not finite), fs.E[9 s ..] the solutions in
// the order of the lanes that hold their roots, a wave_sync behind them.  Called by a whole wave; the result is uniform over it.
__device__ __forceinline__ int five_point_solve(PairScratch &sh, FiveScratch &fs, const double da[3], const double db[3], int lane) {
  {
    double acc[EP_SUMS];
    epipolar_terms(da, db, acc);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < EP_SUMS; i++) {
      acc[i] = wave_all_sum(acc[i]);
      ok = ok && isfinite(acc[i]);
    }
    if (!ok) return 0;
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < EP_SUMS; i++) sh.S[i] = acc[i];
    }
  }
  wave_sync();
  const double tr = epipolar_trace(sh.S);
  for (int e = lane; e < 144; e += 64) sh.rs.M[e] = epipolar_matrix_entry(sh.S, tr, e);
  jacobi12<wave_sync>(sh.rs.M, sh.rs.V, lane, 64);
  {  // lane j < 9 ranks eigenvalue j (ties to the lower index); ranks 0..3 are the basis, 4 is lambda_5, 8 is lambda_9
    const int j = lane < 9 ? lane : 8;
    const double lam = sh.rs.M[13 * j];
    int rank = 0;
    for (int k = 0; k < 9; k++) {
      const double lk = sh.rs.M[13 * k];
      rank += (lk < lam || (lk == lam && k < j)) ? 1 : 0;
    }
    if (__ballot(lane < 9 && !isfinite(lam))) return 0;
    const unsigned long long at5 = __ballot(lane < 9 && rank == 4), at9 = __ballot(lane < 9 && rank == 8);
    if (!at5 || !at9) return 0;
    const double l5 = __shfl(lam, __ffsll((long long)at5) - 1, 64), l9 = __shfl(lam, __ffsll((long long)at9) - 1, 64);
    if (!(l5 > 1e-12 * l9)) return 0;
    if (lane < 9 && rank < 4)
      for (int e = 0; e < 9; e++) fs.N[9 * rank + e] = sh.rs.V[e * 12 + j];
  }
  wave_sync();
  // the coefficient of monomial (a, b, c) in constraint `row`: the form summed over the orders of (a, b, c), each distinct order once
#pragma nounroll
  for (int e = lane; e < FP_ROWS * FP_COLS; e += 64) {
    const int row = e / FP_COLS, code = five_monomial(e % FP_COLS);
    const double *A = fs.N + 9 * (code & 3), *B = fs.N + 9 * ((code >> 2) & 3), *C = fs.N + 9 * ((code >> 4) & 3);
    const double sum = ((((five_form(row, A, B, C) + five_form(row, A, C, B)) + five_form(row, B, A, C)) + five_form(row, B, C, A)) +
                        five_form(row, C, A, B)) + five_form(row, C, B, A);
    const double w = (A == B && B == C) ? 1.0 / 6.0 : ((A == B || B == C) ? 0.5 : 1.0);  // (a <= b <= c)
    fs.C[e] = w * sum;
  }
  wave_sync();
  // Gauss-Jordan with partial pivoting on the first ten columns, lanes over columns
#pragma nounroll
  for (int s = 0; s < FP_ROWS; s++) {
    double col[FP_ROWS];
    int pr = s;
    double big = -1.0;
#pragma unroll
    for (int r = 0; r < FP_ROWS; r++) {
      col[r] = fs.C[r * FP_COLS + s];
      if (r >= s && fabs(col[r]) > big) big = fabs(col[r]), pr = r;
    }
    const double piv = fs.C[pr * FP_COLS + s], head = fs.C[s * FP_COLS + s];
    if (!(fabs(piv) > 0.0) || !isfinite(piv)) return 0;  // (uniform)
    wave_sync();  // (every lane has read column s)
    if (lane < FP_COLS) {
      const double down = fs.C[s * FP_COLS + lane], up = fs.C[pr * FP_COLS + lane] / piv;
#pragma unroll
      for (int r = 0; r < FP_ROWS; r++) {
        if (r == s) continue;
        const double f = r == pr ? head : col[r], old = r == pr ? down : fs.C[r * FP_COLS + lane];
        fs.C[r * FP_COLS + lane] = old - f * up;
      }
      fs.C[s * FP_COLS + lane] = up;
    }
    wave_sync();
  }
  if (lane < 3) {  // row `lane` of B from the rows (4, 5), (6, 7), (8, 9)
    const double *a = fs.C + (4 + 2 * lane) * FP_COLS, *b = a + FP_COLS;
    double *o = fs.B + FP_BROW * lane;
    o[0] = a[12], o[1] = a[11] - b[12], o[2] = a[10] - b[11], o[3] = -b[10];
    o[4] = a[15], o[5] = a[14] - b[15], o[6] = a[13] - b[14], o[7] = -b[13];
    o[8] = a[19], o[9] = a[18] - b[19], o[10] = a[17] - b[18], o[11] = a[16] - b[17], o[12] = -b[16];
  }
  wave_sync();
  if (lane < 11) {  // coefficient `lane` of det B = sum over the rows r of B1_r (Bx_r' By_r'' - Bx_r'' By_r'), (r, r', r'') cyclic
    double v = 0.0;
#pragma nounroll
    for (int r = 0; r < 3; r++) {
      const double *b0 = fs.B + FP_BROW * r, *b1 = fs.B + FP_BROW * ((r + 1) % 3), *b2 = fs.B + FP_BROW * ((r + 2) % 3);
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
          const int k = lane - i - j;
          if (k >= 0 && k <= 4) v += b0[8 + k] * (b1[i] * b2[4 + j] - b2[i] * b1[4 + j]);
        }
    }
    fs.P[lane] = v;
  }
  wave_sync();
  bool fin = true;
  for (int i = 0; i < 11; i++) fin = fin && isfinite(fs.P[i]);
  if (!fin || fs.P[10] == 0.0) return 0;
  // the ten roots, lane k < 10 holds root k: from a circle of the roots' geometric mean modulus
  const int k = lane < 10 ? lane : 9;
  double zr, zi;
  {
    const double g = fabs(fs.P[0] / fs.P[10]);
    const double rad = g > 0.0 ? exp(log(g) / 10.0) : 1.0;
    const double th = 0.4 + 0.62831853071795865 * (double)k;
    zr = rad * cos(th), zi = rad * sin(th);
  }
#pragma nounroll
  for (int it = 0; it < FP_ROOT_ITERS; it++) {
    double pr, pi, dr, di;
    five_horner(fs.P, zr, zi, pr, pi, dr, di);
    const double dn = dr * dr + di * di;
    double wr = (pr * dr + pi * di) / dn, wi = (pi * dr - pr * di) / dn;  // p / p'
    if (pr == 0.0 && pi == 0.0) wr = 0.0, wi = 0.0;
    double sr = 0.0, si = 0.0;  // the sum of 1 / (z_k - z_j) over the other roots
#pragma unroll
    for (int j = 0; j < 10; j++) {
      const double ar = zr - __shfl(zr, j, 64), ai = zi - __shfl(zi, j, 64);
      const double an = ar * ar + ai * ai;
      if (j != k && an > 0.0) sr += ar / an, si -= ai / an;  // (two iterates that coincide do not repel each other)
    }
    const double er = 1.0 - (wr * sr - wi * si), ei = -(wr * si + wi * sr), en = er * er + ei * ei;
    const double stepr = (wr * er + wi * ei) / en, stepi = (wi * er - wr * ei) / en;
    zr -= stepr, zi -= stepi;
    const bool moving = !(stepr * stepr + stepi * stepi <= 1e-20 * (zr * zr + zi * zi));
    if (!__ballot(lane < 10 && moving)) break;
  }
  // a real root: two Newton steps on the real axis, (x, y) from the pair of rows of B(z) whose cross product is the largest
  double E[9];
  bool real = lane < 10 && isfinite(zr) && isfinite(zi) && fabs(zi) <= 1e-7 * sqrt(zr * zr + zi * zi);
  if (real) {
    double z = zr;
#pragma unroll
    for (int it = 0; it < 2; it++) {
      double pr, pi, dr, di;
      five_horner(fs.P, z, 0.0, pr, pi, dr, di);
      const double step = pr / dr;
      if (isfinite(step)) z -= step;
    }
    double b[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double *o = fs.B + FP_BROW * r;
      b[3 * r] = ((o[3] * z + o[2]) * z + o[1]) * z + o[0];
      b[3 * r + 1] = ((o[7] * z + o[6]) * z + o[5]) * z + o[4];
      b[3 * r + 2] = (((o[12] * z + o[11]) * z + o[10]) * z + o[9]) * z + o[8];
    }
    double cx = 0.0, cy = 0.0, cz = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const int r1 = (r + 1) % 3;
      const double x = b[3 * r + 1] * b[3 * r1 + 2] - b[3 * r + 2] * b[3 * r1 + 1];
      const double y = b[3 * r + 2] * b[3 * r1] - b[3 * r] * b[3 * r1 + 2];
      const double w = b[3 * r] * b[3 * r1 + 1] - b[3 * r + 1] * b[3 * r1];
      if (r == 0 || fabs(w) > fabs(cz)) cx = x, cy = y, cz = w;
    }
    double x = cx / cz, y = cy / cz;
    five_polish(fs.C, x, y, z);
    double n2 = 0.0;
#pragma unroll
    for (int e = 0; e < 9; e++) {
      E[e] = ((x * fs.N[e] + y * fs.N[9 + e]) + z * fs.N[18 + e]) + fs.N[27 + e];
      n2 += E[e] * E[e];
    }
    const double nrm = sqrt(n2);
#pragma unroll
    for (int e = 0; e < 9; e++) {
      E[e] = E[e] / nrm;
      real = real && isfinite(E[e]);
    }
  }
  const unsigned long long found = __ballot(real);
  if (real) {
    const int slot = __popcll(found & ((1ull << lane) - 1ull));
#pragma unroll
    for (int e = 0; e < 9; e++) fs.E[9 * slot + e] = E[e];
  }
  wave_sync();
  return __popcll(found);
}

// ---- P3P: the poses of a calibrated camera through three 2D-3D correspondences ---------------------------------------
// Unit rays j_i = (q_i, -1) / |(q_i, -1)|, depths s_i > 0 with R X_i + t = s_i j_i.  The three cosine laws between the points,
// divided by s_1^2 with u = s_2 / s_1 and v = s_3 / s_1, are two quadrics in u whose coefficients are polynomials in v,
//   u^2 + b1 u + c1 = 0,  b1 = -2 cg,    c1 = 1 - (c^2 / b^2) w(v)
//   u^2 + b2 u + c2 = 0,  b2 = -2 ca v,  c2 = v^2 - (a^2 / b^2) w(v),   w(v) = v^2 - 2 cb v + 1
// (a, b, c the sides across X_1, X_2, X_3; ca = j_2.j_3, cb = j_1.j_3, cg = j_1.j_2).  Their resultant in u,
// (c2 - c1)^2 - (b2 - b1) (b1 c2 - b2 c1), is a quartic in v.  Everything lives in the registers of ONE LANE: k_p3p gives every
// lane a problem of its own, and the 64 lanes of a wave of k_ransac_hypotheses_p3p all solve the wave's one sample and hold the
// same bits -- the same code on both paths, no LDS and no exchange between lanes.  All loops over the four roots are unrolled,
// so that no array is indexed by a variable (an indexed private array would go to scratch).
constexpr int P3_POINTS = 3, P3_MAX_SOL = 4, P3_ROOT_ITERS = 100;

// rotation_vector on registers: the same arithmetic with the row of the largest diagonal entry taken by selection, not by
// index.  (A copy: rotation_vector itself works on the LDS of a ResectScratch, and a change to it changes k_resect_cameras.)
__device__ __forceinline__ void rotation_vector_reg(const double R[9], double r[3]) {
  const double w0 = R[7] - R[5], w1 = R[2] - R[6], w2 = R[3] - R[1];
  const double wn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  const double co = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double th = atan2(0.5 * wn, co);
  if (th < 1e-12) {
    r[0] = 1e-12, r[1] = 0.0, r[2] = 0.0;
  } else if (co >= 0.0) {
    r[0] = th * (w0 / wn), r[1] = th * (w1 / wn), r[2] = th * (w2 / wn);
  } else {
    int im = 0;
    double dmax = R[0];
    if (R[4] > dmax) im = 1, dmax = R[4];
    if (R[8] > dmax) im = 2, dmax = R[8];
    const double ki = sqrt((dmax - co) / (1.0 - co));
    // the symmetric part of row im
    const double s0 = im == 0 ? R[0] + R[0] : (im == 1 ? R[3] + R[1] : R[6] + R[2]);
    const double s1 = im == 0 ? R[1] + R[3] : (im == 1 ? R[4] + R[4] : R[7] + R[5]);
    const double s2 = im == 0 ? R[2] + R[6] : (im == 1 ? R[5] + R[7] : R[8] + R[8]);
    r[0] = im == 0 ? ki : 0.5 * s0 / ((1.0 - co) * ki);
    r[1] = im == 1 ? ki : 0.5 * s1 / ((1.0 - co) * ki);
    r[2] = im == 2 ? ki : 0.5 * s2 / ((1.0 - co) * ki);
    const double sgn = (r[0] * w0 + r[1] * w1) + r[2] * w2 < 0.0 ? -1.0 : 1.0;
    const double kn = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    r[0] = th * (sgn * r[0] / kn), r[1] = th * (sgn * r[1] / kn), r[2] = th * (sgn * r[2] / kn);
  }
}

// p(z) and p'(z) of the quartic P (ascending) at the complex z
__device__ __forceinline__ void p3p_horner(const double P[5], double zr, double zi, double &pr, double &pi, double &dr, double &di) {
  pr = P[4], pi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
  for (int i = 3; i >= 0; i--) {
    const double tr = (dr * zr - di * zi) + pr, ti = (dr * zi + di * zr) + pi;
    dr = tr, di = ti;
    const double ur = (pr * zr - pi * zi) + P[i], ui = pr * zi + pi * zr;
    pr = ur, pi = ui;
  }
}

// the orthonormal frame of (p2 - p1, p3 - p1), its vectors the columns of F (row-major): e1 along the first, e3 along their
// cross product, e2 = e3 x e1
__device__ __forceinline__ void p3p_frame(const double p1[3], const double p2[3], const double p3[3], double F[9]) {
  const double a0 = p2[0] - p1[0], a1 = p2[1] - p1[1], a2 = p2[2] - p1[2];
  const double b0 = p3[0] - p1[0], b1 = p3[1] - p1[1], b2 = p3[2] - p1[2];
  const double an = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  const double e10 = a0 / an, e11 = a1 / an, e12 = a2 / an;
  const double n0 = e11 * b2 - e12 * b1, n1 = e12 * b0 - e10 * b2, n2 = e10 * b1 - e11 * b0;
  const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  const double e30 = n0 / nn, e31 = n1 / nn, e32 = n2 / nn;
  const double e20 = e31 * e12 - e32 * e11, e21 = e32 * e10 - e30 * e12, e22 = e30 * e11 - e31 * e10;
  F[0] = e10, F[1] = e20, F[2] = e30;
  F[3] = e11, F[4] = e21, F[5] = e31;
  F[6] = e12, F[7] = e22, F[8] = e32;
}

// The poses through the three correspondences (q_i, X_i): q the undistorted image points, already divided by f.  pose[k], k in
// 0..3: r and t of the solution at the k-th real root of the quartic in ascending order (the complex ones last); returns the
// mask of the k whose pose is a solution (v > 0, u > 0, every component finite) -- 0 for a side that is 0 or not finite, three
// points on a line (|(X2 - X1) x (X3 - X1)| <= 1e-12 c b), a quartic that is not finite or has no leading coefficient.  The
// caller takes the set bits in ascending k.  (one lane)
__device__ __forceinline__ unsigned p3p_solve(const double q[P3_POINTS][2], const double X[P3_POINTS][3], double pose[P3_MAX_SOL][6]) {
  double j[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double n = sqrt((q[i][0] * q[i][0] + q[i][1] * q[i][1]) + 1.0);
    j[i][0] = q[i][0] / n, j[i][1] = q[i][1] / n, j[i][2] = -1.0 / n;
  }
  double e21[3], e31[3], e32[3];
#pragma unroll
  for (int i = 0; i < 3; i++) e21[i] = X[1][i] - X[0][i], e31[i] = X[2][i] - X[0][i], e32[i] = X[2][i] - X[1][i];
  const double a = sqrt((e32[0] * e32[0] + e32[1] * e32[1]) + e32[2] * e32[2]);
  const double b = sqrt((e31[0] * e31[0] + e31[1] * e31[1]) + e31[2] * e31[2]);
  const double c = sqrt((e21[0] * e21[0] + e21[1] * e21[1]) + e21[2] * e21[2]);
  if (!(a > 0.0) || !(b > 0.0) || !(c > 0.0) || !isfinite(a) || !isfinite(b) || !isfinite(c)) return 0u;
  {
    const double n0 = e21[1] * e31[2] - e21[2] * e31[1], n1 = e21[2] * e31[0] - e21[0] * e31[2], n2 = e21[0] * e31[1] - e21[1] * e31[0];
    if (!(sqrt((n0 * n0 + n1 * n1) + n2 * n2) > 1e-12 * c * b)) return 0u;
  }
  const double ca = (j[1][0] * j[2][0] + j[1][1] * j[2][1]) + j[1][2] * j[2][2];
  const double cb = (j[0][0] * j[2][0] + j[0][1] * j[2][1]) + j[0][2] * j[2][2];
  const double cg = (j[0][0] * j[1][0] + j[0][1] * j[1][1]) + j[0][2] * j[1][2];
  const double A = (c * c) / (b * b), B = (a * a) / (b * b);
  // c1, c2 (ascending in v); D = c2 - c1; E = b2 - b1 = E0 + E1 v; G = b1 c2 - b2 c1
  const double c1[3] = {1.0 - A, 2.0 * A * cb, -A}, c2[3] = {-B, 2.0 * B * cb, 1.0 - B};
  const double D[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
  const double E0 = 2.0 * cg, E1 = -2.0 * ca;
  const double G[4] = {-E0 * c2[0], -E0 * c2[1] - E1 * c1[0], -E0 * c2[2] - E1 * c1[1], -E1 * c1[2]};
  double P[5];
  P[0] = D[0] * D[0] - E0 * G[0];
  P[1] = 2.0 * (D[0] * D[1]) - (E0 * G[1] + E1 * G[0]);
  P[2] = (2.0 * (D[0] * D[2]) + D[1] * D[1]) - (E0 * G[2] + E1 * G[1]);
  P[3] = 2.0 * (D[1] * D[2]) - (E0 * G[3] + E1 * G[2]);
  P[4] = D[2] * D[2] - E1 * G[3];
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 5; i++) fin = fin && isfinite(P[i]);
  if (!fin || P[4] == 0.0) return 0u;
  // the four roots by the simultaneous iteration of Aberth and Ehrlich, from a circle of their geometric mean modulus
  double zr[4], zi[4];
  {
    const double g = fabs(P[0] / P[4]);
    const double rad = g > 0.0 ? exp(log(g) / 4.0) : 1.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double th = 0.4 + 1.5707963267948966 * (double)k;
      zr[k] = rad * cos(th), zi[k] = rad * sin(th);
    }
  }
#pragma nounroll
  for (int it = 0; it < P3_ROOT_ITERS; it++) {
    double stepr[4], stepi[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      double pr, pi, dr, di;
      p3p_horner(P, zr[k], zi[k], pr, pi, dr, di);
      const double dn = dr * dr + di * di;
      double wr = (pr * dr + pi * di) / dn, wi = (pi * dr - pr * di) / dn;  // p / p'
      if (pr == 0.0 && pi == 0.0) wr = 0.0, wi = 0.0;
      double sr = 0.0, si = 0.0;  // the sum of 1 / (z_k - z_j) over the other roots
#pragma unroll
      for (int l = 0; l < 4; l++) {
        if (l == k) continue;
        const double ar = zr[k] - zr[l], ai = zi[k] - zi[l];
        const double an = ar * ar + ai * ai;
        if (an > 0.0) sr += ar / an, si -= ai / an;  // (two iterates that coincide do not repel each other)
      }
      const double er = 1.0 - (wr * sr - wi * si), ei = -(wr * si + wi * sr), en = er * er + ei * ei;
      stepr[k] = (wr * er + wi * ei) / en, stepi[k] = (wi * er - wr * ei) / en;
    }
    bool moving = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      zr[k] -= stepr[k], zi[k] -= stepi[k];
      moving = moving || !(stepr[k] * stepr[k] + stepi[k] * stepi[k] <= 1e-20 * (zr[k] * zr[k] + zi[k] * zi[k]));
    }
    if (!moving) break;
  }
  // a real root takes two Newton steps on the real axis; a complex one sorts last
  const double inf = __builtin_inf();
  double v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool real = isfinite(zr[k]) && isfinite(zi[k]) && fabs(zi[k]) <= 1e-7 * sqrt(zr[k] * zr[k] + zi[k] * zi[k]);
    double z = zr[k];
#pragma unroll
    for (int it = 0; it < 2; it++) {
      double pr, pi, dr, di;
      p3p_horner(P, z, 0.0, pr, pi, dr, di);
      const double step = pr / dr;
      if (isfinite(step)) z -= step;
    }
    v[k] = real ? z : inf;
  }
#define P3_ORDER(i, k)                 \
  {                                    \
    const double lo = v[i], hi = v[k]; \
    const bool sw = lo > hi;           \
    v[i] = sw ? hi : lo;               \
    v[k] = sw ? lo : hi;               \
  }
  P3_ORDER(0, 1) P3_ORDER(2, 3) P3_ORDER(0, 2) P3_ORDER(1, 3) P3_ORDER(1, 2)
#undef P3_ORDER
  double Fw[9];
  p3p_frame(X[0], X[1], X[2], Fw);
  const double a2 = a * a, b2 = b * b, cc2 = c * c;
  unsigned found = 0u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vk = v[k];
    if (!(vk < inf)) continue;  // (a complex root: uniform over the wave of a hypothesis, which all hold the same roots)
    bool ok = true;
    const double wv = (vk * vk - 2.0 * cb * vk) + 1.0;
    const double c1v = 1.0 - A * wv, c2v = vk * vk - B * wv;
    const double den = -(E0 + E1 * vk);  // b1 - b2
    double u = (c2v - c1v) / den;
    if (den == 0.0 || !isfinite(u)) {  // the root of the first quadric that satisfies the second better
      const double disc = cg * cg - c1v, sq = sqrt(disc > 0.0 ? disc : 0.0);
      const double ua = cg + sq, ub = cg - sq;
      const double fa = fabs((ua * ua - 2.0 * ca * vk * ua) + c2v), fb = fabs((ub * ub - 2.0 * ca * vk * ub) + c2v);
      u = fb < fa ? ub : ua;
    }
    ok = ok && vk > 0.0 && u > 0.0;
    double s1 = b / sqrt(wv), s2 = u * s1, s3 = vk * s1;
    // two Gauss-Newton steps on the three cosine laws
#pragma unroll
    for (int it = 0; it < 2; it++) {
      const double f1 = ((s2 * s2 + s3 * s3) - 2.0 * ca * (s2 * s3)) - a2;
      const double f2 = ((s1 * s1 + s3 * s3) - 2.0 * cb * (s1 * s3)) - b2;
      const double f3 = ((s1 * s1 + s2 * s2) - 2.0 * cg * (s1 * s2)) - cc2;
      // J = 2 [[0, m01, m02], [m10, 0, m12], [m20, m21, 0]]
      const double m01 = s2 - ca * s3, m02 = s3 - ca * s2;
      const double m10 = s1 - cb * s3, m12 = s3 - cb * s1;
      const double m20 = s1 - cg * s2, m21 = s2 - cg * s1;
      const double det = 2.0 * (m01 * (m12 * m20) + m02 * (m10 * m21));
      const double d1 = ((-(m12 * m21)) * f1 + (m02 * m21) * f2 + (m01 * m12) * f3) / det;
      const double d2 = ((m12 * m20) * f1 + (-(m02 * m20)) * f2 + (m02 * m10) * f3) / det;
      const double d3 = ((m10 * m21) * f1 + (m01 * m20) * f2 + (-(m01 * m10)) * f3) / det;
      if (isfinite(d1) && isfinite(d2) && isfinite(d3)) s1 -= d1, s2 -= d2, s3 -= d3;
    }
    const double Y1[3] = {s1 * j[0][0], s1 * j[0][1], s1 * j[0][2]};
    const double Y2[3] = {s2 * j[1][0], s2 * j[1][1], s2 * j[1][2]};
    const double Y3[3] = {s3 * j[2][0], s3 * j[2][1], s3 * j[2][2]};
    double Fc[9], R[9];
    p3p_frame(Y1, Y2, Y3, Fc);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int l = 0; l < 3; l++) R[3 * i + l] = (Fc[3 * i] * Fw[3 * l] + Fc[3 * i + 1] * Fw[3 * l + 1]) + Fc[3 * i + 2] * Fw[3 * l + 2];
    rotation_vector_reg(R, pose[k]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      pose[k][3 + i] = Y1[i] - ((R[3 * i] * X[0][0] + R[3 * i + 1] * X[0][1]) + R[3 * i + 2] * X[0][2]);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && isfinite(pose[k][i]);
    if (ok) found |= 1u << k;
  }
  return found;
}

// ---- the non-linear refinement of a pair: Marquardt steps on the signed Sampson residual in 5 unknowns -------------
// The pose is (R, unit t); a step is delta = (d_omega, d_tau): R+ = exp([d_omega]x) R, t+ = (t + B d_tau) / |t + B d_tau| with
// B = [b1 b2] a basis of the plane across t.  The residual of a match is e = n / sqrt(D), n = d_b' E d_a,
// D = ((E d_a)_1^2 + (E d_a)_2^2) / f_b^2 + ((E' d_b)_1^2 + (E' d_b)_2^2) / f_a^2: e^2 is the Sampson distance of pair_inlier.
// With dE = G for a unit step in one unknown, dn = d_b' G d_a, d(E d_a) = G d_a, d(E' d_b) = G' d_b, and
// de = dn / sqrt(D) - n dD / (2 D^(3/2)).  The five G of a pose are G_omega_j = [t]x [e_j]x R and G_tau_j = [b_j]x R
// (pair_tangent): one lane writes them when the pose moves, every lane reads them for each of its matches.
constexpr int RP_DOF = 5;
constexpr int RP_HESS = RP_DOF * (RP_DOF + 1) / 2;  // H packed lower row-major
constexpr int RP_SUMS = 1 + RP_DOF + RP_HESS;      // F, g, H
constexpr int RP_MIN_SET = RP_DOF;                 // the smallest set that is refined

// e of a match under E (row-major); l <- the first two entries of E d_a, m <- of E' d_b, n and D as above
__device__ __forceinline__ double pair_sampson_signed(const double *ray, const double *E, double fa, double fb, double l[2], double m[2],
                                                      double &n, double &D) {
  const double qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
  l[0] = (E[0] * qax + E[1] * qay) - E[2], l[1] = (E[3] * qax + E[4] * qay) - E[5];
  const double l2 = (E[6] * qax + E[7] * qay) - E[8];
  m[0] = (E[0] * qbx + E[3] * qby) - E[6], m[1] = (E[1] * qbx + E[4] * qby) - E[7];
  n = (qbx * l[0] + qby * l[1]) - l2;
  D = (l[0] * l[0] + l[1] * l[1]) / (fb * fb) + (m[0] * m[0] + m[1] * m[1]) / (fa * fa);
  return n / sqrt(D);
}

// J[j] <- de / d delta_j of the match from the five G (9 entries each, row-major) and what pair_sampson_signed left
__device__ __forceinline__ void pair_sampson_jacobian(const double *ray, const double *G, double fa, double fb, const double l[2],
                                                      const double m[2], double n, double D, double J[RP_DOF]) {
  const double qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
  const double rD = sqrt(D), half = n / (2.0 * (D * rD));
#pragma unroll
  for (int j = 0; j < RP_DOF; j++) {
    const double *g = G + 9 * j;
    const double dl0 = (g[0] * qax + g[1] * qay) - g[2], dl1 = (g[3] * qax + g[4] * qay) - g[5], dl2 = (g[6] * qax + g[7] * qay) - g[8];
    const double dm0 = (g[0] * qbx + g[3] * qby) - g[6], dm1 = (g[1] * qbx + g[4] * qby) - g[7];
    const double dn = (qbx * dl0 + qby * dl1) - dl2;
    const double dD = 2.0 * (l[0] * dl0 + l[1] * dl1) / (fb * fb) + 2.0 * (m[0] * dm0 + m[1] * dm1) / (fa * fa);
    J[j] = dn / rD - half * dD;
  }
}

// out (row-major 3 x 3) <- [v]x R
__device__ __forceinline__ void cross_rows(const double *v, const double *R, double *out) {
  for (int c = 0; c < 3; c++) {
    out[c] = v[1] * R[6 + c] - v[2] * R[3 + c];
    out[3 + c] = v[2] * R[c] - v[0] * R[6 + c];
    out[6 + c] = v[0] * R[3 + c] - v[1] * R[c];
  }
}

// The basis B of the plane across t and the five G of the pose (R, t) -> B (b1, b2), G; W: 9 doubles of scratch.  b1 = (e_i x t)
// / |e_i x t| with i the index of the smallest |t_i|, ties to the lowest; b2 = t x b1.  (one lane, on LDS)
__device__ __forceinline__ void pair_tangent(const double *R, const double *t, double *B, double *G, double *W) {
  int i = 0;
  if (fabs(t[1]) < fabs(t[i])) i = 1;
  if (fabs(t[2]) < fabs(t[i])) i = 2;
  const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;  // e_i x t = -t_{i+2} e_{i+1} + t_{i+1} e_{i+2}
  const double bn = sqrt(t[i1] * t[i1] + t[i2] * t[i2]);
  B[i] = 0.0, B[i1] = -t[i2] / bn, B[i2] = t[i1] / bn;
  B[3] = t[1] * B[2] - t[2] * B[1], B[4] = t[2] * B[0] - t[0] * B[2], B[5] = t[0] * B[1] - t[1] * B[0];
  for (int j = 0; j < 3; j++) {
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    cross_rows(e, R, W);
    cross_rows(t, W, G + 9 * j);
  }
  cross_rows(B, R, G + 27);
  cross_rows(B + 3, R, G + 36);
}

// (R, t) moved by delta -> Rn, tn, En = [tn]x Rn; exp([w]x) = I + a [w]x + b [w]x^2 with a = sin(th) / th and
// b = (sin(th / 2) / (th / 2))^2 / 2, th = |w| (th == 0: a = 1, b = 1 / 2).  (one lane, on LDS)
__device__ __forceinline__ void pair_retract(const double *R, const double *t, const double *B, const double *delta, double *Rn, double *tn,
                                             double *En, double *W) {
  const double w[3] = {delta[0], delta[1], delta[2]};
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  double ca = 1.0, cb = 0.5;
  if (th > 0.0) {
    const double sh = sin(0.5 * th) / (0.5 * th);
    ca = sin(th) / th, cb = 0.5 * (sh * sh);
  }
  cross_rows(w, R, W);    // [w]x R
  cross_rows(w, W, Rn);   // [w]x^2 R
  for (int e = 0; e < 9; e++) Rn[e] = (R[e] + ca * W[e]) + cb * Rn[e];
  double u[3];
  for (int i = 0; i < 3; i++) u[i] = (t[i] + B[i] * delta[3]) + B[3 + i] * delta[4];
  const double un = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  // (a step too small to move t leaves its bits: the retraction of 0 is the identity, also where |t| is an ulp off 1 -- without
  // this a t whose renormalised copy costs an ulp more rejects every trial from there on and the pair ends STALLED at its minimum)
  const bool still = u[0] == t[0] && u[1] == t[1] && u[2] == t[2];
  for (int i = 0; i < 3; i++) tn[i] = still ? t[i] : u[i] / un;
  cross_rows(tn, Rn, En);
}

// (H + lam diag H) delta = -g by Cholesky; S: the sums (F, g, H packed lower row-major); L: 15 doubles of scratch.  false: a pivot
// that is not > 0 or a delta that is not finite.  (one lane, on LDS)
__device__ __forceinline__ bool pair_step(const double *S, double lam, double *L, double *delta) {
  const double *g = S + 1, *H = S + 1 + RP_DOF;
#pragma nounroll
  for (int i = 0; i < RP_DOF; i++)
#pragma nounroll
    for (int j = 0; j <= i; j++) {
      double s = H[i * (i + 1) / 2 + j];
      if (i == j) s += lam * s;
      for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      if (i == j) {
        if (!(s > 0.0) || !isfinite(s)) return false;
        L[i * (i + 1) / 2 + i] = sqrt(s);
      } else {
        L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
      }
    }
#pragma nounroll
  for (int i = 0; i < RP_DOF; i++) {  // L y = -g
    double s = -g[i];
    for (int k = 0; k < i; k++) s -= L[i * (i + 1) / 2 + k] * delta[k];
    delta[i] = s / L[i * (i + 1) / 2 + i];
  }
  bool ok = true;
#pragma nounroll
  for (int i = RP_DOF - 1; i >= 0; i--) {  // L' delta = y
    double s = delta[i];
    for (int k = i + 1; k < RP_DOF; k++) s -= L[k * (k + 1) / 2 + i] * delta[k];
    delta[i] = s / L[i * (i + 1) / 2 + i];
    ok = ok && isfinite(delta[i]);
  }
  return ok;
}
