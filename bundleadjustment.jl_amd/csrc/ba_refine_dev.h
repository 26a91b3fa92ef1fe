// Device pieces shared by the block refinements (ba_point_kernels.hip, ba_camera_kernels.hip, ba_ransac_kernels.hip; DESIGN
// §5j-§5m).  Included inside the including file's unnamed namespace; gfx950 only.  These files are built without FMA contraction:
// the operand order and the parentheses here are those of the model's device functions and must stay.
//
// Two more pieces are alike in both files and stay written out at their sites, because as shared functions they change the
// kernels' instructions (tools/compare_code_objects.py against the build before): the load of an observation's information
// factors with its "Lambda == 0" test (load_obs; observation_sums and obs_used) and the undistortion loop (point_triangulate;
// k_resect_cameras), which share only its iteration count.
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

// ---- pieces of the linear resection (k_resect_cameras; the hypotheses of ba_ransac_cameras) ----------------------------------
// Sh: the LDS block of the caller, with the members W[9], V3[9], sg[3], U[9], R[9], r[3]
constexpr int RS_SWEEPS = 30;       // cap of the Jacobi sweeps (12 x 12 and 3 x 3)

// The nearest proper rotation of the 3 x 3 matrix sh.W (row-major) -> sh.R, its singular values -> sh.sg: one-sided Jacobi
// (rotations of column pairs until they are orthogonal: W V3 = U Sigma), then R = U diag(1, 1, det(U V3')) V3' with the sign on
// the smallest singular value -- its column of U is taken as the cross product of the other two, which is that sign and
// needs no division by a singular value that may be 0.  (one lane)
template <typename Sh>
__device__ __forceinline__ void nearest_rotation(Sh &sh) {
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
template <typename Sh>
__device__ __forceinline__ void rotation_vector(Sh &sh) {
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
