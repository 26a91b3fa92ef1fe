// Device functions of the BAL camera model shared by the kernels that evaluate it (ba_model_kernels.hip, ba_point_kernels.hip):
// the per-camera row (cam_pre), the projection from it (project_pre) and the hand-derived 2 x 12 Jacobian block (jac_block).
// Included inside the including file's unnamed namespace; gfx950 only.
#pragma once

template <typename T>
struct Trig;
template <>
struct Trig<double> {
  static __device__ inline void sc(double th, double &s, double &c) { sincos(th, &s, &c); }
  static __device__ inline double sq(double v) { return sqrt(v); }
};
template <>
struct Trig<float> {
  // Julia's Float32 sin/cos round a double-precision kernel once; do the same.
  static __device__ inline void sc(float th, float &s, float &c) {
    double sd, cd;
    sincos((double)th, &sd, &cd);
    s = (float)sd;
    c = (float)cd;
  }
  static __device__ inline float sq(float v) { return sqrtf(v); }
};

constexpr int CPAD = 16;  // precomputed camera rows: 16 elements (one 128-byte line for double), 16-byte aligned

// 2x12 block of one observation: denseJ = (JP3*JP2)*JP1 evaluated without the structural zeros of the
// reference's padded 2x5 / 5x6 / 6x12 matrices (BALNLPModels.jl:177-197).  Entries of JP1/JP2/JP3 are
// computed in T, the chain products in double (for T = Float32 the reference's scratch matrices are
// Float64, BALNLPModels.jl:177,179).  Column order [X(3), r(3), t(3), k1, k2, f].
// Unlike the residual (which keeps the reference's operation order), this block is tolerance-matched by
// contract (the reference's own values depend on OpenBLAS' summation order, SURVEY.md 8c: <= 1e-12 of the
// block inf-norm), so the ten divisions by theta and z are two reciprocals and a*b+c contracts to FMA.
// The part of the block that depends on the camera only (theta, the unit axis, sin and cos): evaluated once per camera
// by k_cam_pre instead of once per observation.  Row layout (CPAD = 16 elements, one 128-byte line for double):
//   [kx ky kz | t(3) | k1 k2 f | sin cos 1/theta | 0 0 0 0]
template <typename T>
__device__ inline void cam_pre(const T C[9], T P[12]) {
  // theta, the axis, sin and cos in the reference's operation order (BALNLPModels.jl:19-22: sqrt of the left-folded sum,
  // three divisions, no contraction; no theta -> 0 guard: the reference has none): the residual takes them from this
  // row, and evaluating them once per camera instead of once per observation changes no bit.  1/theta is for the
  // Jacobian only.
  const T th = Trig<T>::sq(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
  T s, c;
  Trig<T>::sc(th, s, c);
  P[0] = C[0] / th;
  P[1] = C[1] / th;
  P[2] = C[2] / th;
#pragma unroll
  for (int i = 3; i < 9; i++) P[i] = C[i];
  P[9] = s;
  P[10] = c;
  P[11] = (T)1 / th;
}

// projection!  src/BALNLPModels.jl:17-33 from a cam_pre row, in the reference's evaluation order (left folds; no z == 0
// guard: the reference has none).  scaling_factor: the literal 1.0 is a Float64 (BALNLPModels.jl:13) -> promoted for
// T = Float32.
template <typename T>
__device__ inline void project_pre(const T X[3], const T P[12], T out[2]) {
  const T k0 = P[0], k1 = P[1], k2 = P[2], s = P[9], c = P[10];
  T kx0 = k1 * X[2] - k2 * X[1];
  T kx1 = k2 * X[0] - k0 * X[2];
  T kx2 = k0 * X[1] - k1 * X[0];
  T d = k0 * X[0] + k1 * X[1] + k2 * X[2];
  T omc_d = (1 - c) * d;
  T P1[3], P2[2];
  P1[0] = ((c * X[0] + s * kx0) + omc_d * k0) + P[3];
  P1[1] = ((c * X[1] + s * kx1) + omc_d * k1) + P[4];
  P1[2] = ((c * X[2] + s * kx2) + omc_d * k2) + P[5];
  P2[0] = -P1[0] / P1[2];
  P2[1] = -P1[1] / P1[2];
  T sqn = P2[0] * P2[0] + P2[1] * P2[1];
  double sc = (1.0 + (double)(P[6] * sqn)) + (double)(P[7] * (sqn * sqn));
  double fs = (double)P[8] * sc;
  out[0] = (T)(fs * (double)P2[0]);
  out[1] = (T)(fs * (double)P2[1]);
}

template <typename T>
__device__ inline void jac_block(const T X[3], const T P[12], T J[24]) {
#pragma clang fp contract(fast)
  const T x = X[0], y = X[1], z = X[2];
  const T kx = P[0], ky = P[1], kz = P[2];
  const T s = P[9], c = P[10], ith = P[11];
  const T *C = P;  // C[3..8] = t, k1, k2, f as in the camera block
  const T d = kx * x + ky * y + kz * z;
  const T omc = 1 - c;
  const T omc_d = omc * d;
  T P1[3], P2[2];
  P1[0] = ((c * x + s * (ky * z - kz * y)) + omc_d * kx) + C[3];
  P1[1] = ((c * y + s * (kz * x - kx * z)) + omc_d * ky) + C[4];
  P1[2] = ((c * z + s * (kx * y - ky * x)) + omc_d * kz) + C[5];
  const T iz = (T)1 / P1[2];
  P2[0] = -P1[0] * iz;
  P2[1] = -P1[1] * iz;
  const T sth = s * ith, omcth = omc * ith;
  const T kx2 = kx * kx, ky2 = ky * ky, kz2 = kz * kz;
  // JP1!  JacobianByHand.jl:27-59: R = d(P1)/dX (3x3), G = d(P1)/dr (3x3)
  T R[3][3], G[3][3];
  R[0][0] = c + omc * kx2;
  R[0][1] = -s * kz + omc * ky * kx;
  R[0][2] = s * ky + omc * kz * kx;
  G[0][0] = -s * x * kx + c * kx * (ky * z - kz * y) + sth * (-ky * kx * z + kz * kx * y) + s * kx2 * d +
            omcth * (2 * x * kx * (1 - kx2) + y * ky * (1 - 2 * kx2) + z * kz * (1 - 2 * kx2));
  G[0][1] = -s * x * ky + c * ky * (ky * z - kz * y) + sth * ((1 - ky2) * z + kz * ky * y) + s * kx * ky * d +
            omcth * (-2 * x * kx2 * ky + y * kx * (1 - 2 * ky2) - 2 * z * kx * ky * kz);
  G[0][2] = -s * x * kz + c * kz * (ky * z - kz * y) + sth * (-ky * kz * z - (1 - kz2) * y) + s * kx * kz * d +
            omcth * (-2 * x * kx2 * kz - 2 * y * kx * ky * kz + z * kx * (1 - 2 * kz2));
  R[1][0] = s * kz + omc * ky * kx;
  R[1][1] = c + omc * ky2;
  R[1][2] = -s * kx + omc * ky * kz;
  G[1][0] = -s * y * kx + c * kx * (kz * x - kx * z) + sth * (-kz * kx * x - (1 - kx2) * z) + s * kx * ky * d +
            omcth * (x * ky * (1 - 2 * kx2) - 2 * y * kx * ky2 - 2 * z * kx * ky * kz);
  G[1][1] = -s * y * ky + c * ky * (kz * x - kx * z) + sth * (-kz * ky * x + kx * ky * z) + s * ky2 * d +
            omcth * (x * kx * (1 - 2 * ky2) + 2 * y * ky * (1 - ky2) + z * kz * (1 - 2 * ky2));
  G[1][2] = -s * y * kz + c * kz * (kz * x - kx * z) + sth * ((1 - kz2) * x + kx * kz * z) + s * kz * ky * d +
            omcth * (-2 * x * kx * ky * kz - 2 * y * ky2 * kz + z * ky * (1 - 2 * kz2));
  R[2][0] = -s * ky + omc * kx * kz;
  R[2][1] = s * kx + omc * ky * kz;
  R[2][2] = c + omc * kz2;
  G[2][0] = -s * z * kx + c * kx * (kx * y - ky * x) + sth * ((1 - kx2) * y + kx * ky * x) + s * kx * kz * d +
            omcth * (x * kz * (1 - 2 * kx2) - 2 * y * kx * ky * kz - 2 * z * kx * kz2);
  G[2][1] = -s * z * ky + c * ky * (kx * y - ky * x) + sth * (-kx * ky * y - (1 - ky2) * x) + s * ky * kz * d +
            omcth * (-2 * x * kx * ky * kz + y * kz * (1 - 2 * ky2) - 2 * z * ky * kz2);
  G[2][2] = -s * z * kz + c * kz * (kx * y - ky * x) + sth * (-kx * kz * y + kz * ky * x) + s * kz2 * d +
            omcth * (x * kx * (1 - 2 * kz2) + y * ky * (1 - 2 * kz2) + 2 * z * kz * (1 - kz2));
  // JP2!  JacobianByHand.jl:62-77
  const T a = -iz;
  const T b0 = P1[0] * iz * iz;
  const T b1 = P1[1] * iz * iz;
  // JP3!  JacobianByHand.jl:80-101
  const T k1 = C[6], k2 = C[7], f = C[8];
  const T xx = P2[0], yy = P2[1];
  const T norm2 = xx * xx + yy * yy;
  const T norm4 = norm2 * norm2;
  const T rr = 1 + k1 * norm2 + k2 * norm4;
  const T gx = 2 * k1 * xx + k2 * (4 * (xx * xx * xx) + 4 * xx * (yy * yy));
  const T gy = 2 * k1 * yy + k2 * (4 * (yy * yy * yy) + 4 * yy * (xx * xx));
  T JP3[2][5];
  JP3[0][0] = f * rr + f * gx * xx;
  JP3[0][1] = f * gy * xx;
  JP3[0][2] = f * norm2 * xx;
  JP3[0][3] = f * norm4 * xx;
  JP3[0][4] = rr * xx;
  JP3[1][0] = f * gx * yy;
  JP3[1][1] = f * rr + f * gy * yy;
  JP3[1][2] = f * norm2 * yy;
  JP3[1][3] = f * norm4 * yy;
  JP3[1][4] = rr * yy;
  const bool z_zero = (P1[2] == 0);  // P2()/JP2!() return NaN there: the whole block is NaN -> 0 (BALNLPModels.jl:201)
#pragma unroll
  for (int q = 0; q < 2; q++) {
    double M0 = (double)JP3[q][0] * (double)a;
    double M1 = (double)JP3[q][1] * (double)a;
    double M2 = (double)JP3[q][0] * (double)b0 + (double)JP3[q][1] * (double)b1;
    double v[12];
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      v[cc] = (M0 * (double)R[0][cc] + M1 * (double)R[1][cc]) + M2 * (double)R[2][cc];
      v[3 + cc] = (M0 * (double)G[0][cc] + M1 * (double)G[1][cc]) + M2 * (double)G[2][cc];
    }
    v[6] = M0;
    v[7] = M1;
    v[8] = M2;
    v[9] = (double)JP3[q][2];
    v[10] = (double)JP3[q][3];
    v[11] = (double)JP3[q][4];
#pragma unroll
    for (int cc = 0; cc < 12; cc++) {
      T t = (T)v[cc];
      J[12 * q + cc] = (z_zero || t != t) ? (T)0 : t;
    }
  }
}
