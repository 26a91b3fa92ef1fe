// Device function of the centre priors shared by the kernels that evaluate it (ba_prior_kernels.hip, ba_camera_kernels.hip): the
// camera centre and its 3 x 6 Jacobian.  Included inside the including file's unnamed namespace; gfx950 only.
#pragma once

// Camera centre c = -R(r)' t of the camera block C = (r, t, ...): R the model's Rodrigues rotation with theta = |r| and the
// unit axis k = r / theta evaluated as cam_pre does (ba_model_kernels.hip: no theta -> 0 branch, the model has none), so
// R' t = cos t - sin (k x t) + (1 - cos) (k.t) k.  LIN: H = dc/d(r, t), 3 x 6 row-major, by hand: dc/dt = -R'; column j of
// d(R't)/dr from dtheta/dr_j = k_j and dk/dr_j = (e_j - k_j k) / theta.
template <bool LIN>
__device__ __forceinline__ void centre_of(const double *__restrict__ C, double c[3], double H[18]) {
  const double th = sqrt(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
  double s, a;
  sincos(th, &s, &a);
  const double k[3] = {C[0] / th, C[1] / th, C[2] / th}, t[3] = {C[3], C[4], C[5]};
  const double kt[3] = {k[1] * t[2] - k[2] * t[1], k[2] * t[0] - k[0] * t[2], k[0] * t[1] - k[1] * t[0]};
  const double d = k[0] * t[0] + k[1] * t[1] + k[2] * t[2], m = 1.0 - a;
#pragma unroll
  for (int i = 0; i < 3; i++) c[i] = -((a * t[i] - s * kt[i]) + m * d * k[i]);
  if (LIN) {
    const double ith = 1.0 / th;
    const double kx[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};  // [k]x
    const double ext[3][3] = {{0.0, -t[2], t[1]}, {t[2], 0.0, -t[0]}, {-t[1], t[0], 0.0}};  // ext[j] = e_j x t
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double base = (-s * t[i] - a * kt[i]) + s * d * k[i];
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double dij = i == j ? 1.0 : 0.0;
        const double dv = k[j] * base - s * ith * (ext[j][i] - k[j] * kt[i]) +
                          m * ith * ((t[j] - k[j] * d) * k[i] + d * (dij - k[j] * k[i]));
        H[6 * i + j] = -dv;
        H[6 * i + 3 + j] = -((a * dij - s * kx[i][j]) + m * k[i] * k[j]);
      }
    }
  }
}
