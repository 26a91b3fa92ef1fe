// Device pieces of rotation averaging (ba_rotavg_kernels.hip): 3 x 3 rotations in nine scalars each.  Included
// inside the including file's unnamed namespace, after ba_refine_dev.h; gfx950 only; built without FMA contraction.  A matrix is
// a double[9], row-major, that is only ever indexed by constants and only passed to functions that are forced inline, so it
// lives in registers (an array indexed by a variable would go to scratch: tests/test_code_objects.py).
#pragma once

// R <- the 3 x 3 at g, or its transpose
__device__ __forceinline__ void mat3_load(const double *__restrict__ g, bool transpose, double R[9]) {
  const double a1 = g[1], a2 = g[2], a3 = g[3], a5 = g[5], a6 = g[6], a7 = g[7];
  R[0] = g[0], R[4] = g[4], R[8] = g[8];
  R[1] = transpose ? a3 : a1, R[3] = transpose ? a1 : a3;
  R[2] = transpose ? a6 : a2, R[6] = transpose ? a2 : a6;
  R[5] = transpose ? a7 : a5, R[7] = transpose ? a5 : a7;
}

// C <- A B
__device__ __forceinline__ void mat3_mul(const double A[9], const double B[9], double C[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
  }
}

// C <- A B'
__device__ __forceinline__ void mat3_mul_bt(const double A[9], const double B[9], double C[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2];
  }
}

// the angle of a rotation matrix by the formula of rotation_vector: atan2(|w| / 2, (tr M - 1) / 2), w the skew part
__device__ __forceinline__ double mat3_angle(const double M[9]) {
  const double w0 = M[7] - M[5], w1 = M[2] - M[6], w2 = M[3] - M[1];
  const double wn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  return atan2(0.5 * wn, 0.5 * (((M[0] + M[4]) + M[8]) - 1.0));
}

// Exp: Rodrigues, cos I + sin [k]x + (1 - cos) k k' with k = v / |v|; |v| = 0 gives I
__device__ __forceinline__ void rotavg_exp(double v0, double v1, double v2, double R[9]) {
  const double th = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  if (th == 0.0) {
    R[0] = 1.0, R[1] = 0.0, R[2] = 0.0, R[3] = 0.0, R[4] = 1.0, R[5] = 0.0, R[6] = 0.0, R[7] = 0.0, R[8] = 1.0;
    return;
  }
  const double k0 = v0 / th, k1 = v1 / th, k2 = v2 / th;
  const double s = sin(th), c = cos(th), u = 1.0 - c;
  R[0] = c + u * (k0 * k0), R[1] = u * (k0 * k1) - s * k2, R[2] = u * (k0 * k2) + s * k1;
  R[3] = u * (k1 * k0) + s * k2, R[4] = c + u * (k1 * k1), R[5] = u * (k1 * k2) - s * k0;
  R[6] = u * (k2 * k0) - s * k1, R[7] = u * (k2 * k1) + s * k0, R[8] = c + u * (k2 * k2);
}

// Log: the rotation vector of M by rotation_vector_reg (its branch near pi included), with 0 where that rule writes its
// (1e-12, 0, 0) for the identity
__device__ __forceinline__ void rotavg_log(const double M[9], double v[3]) {
  const double th = mat3_angle(M);
  rotation_vector_reg(M, v);
  if (th < 1e-12) v[0] = 0.0, v[1] = 0.0, v[2] = 0.0;
}
