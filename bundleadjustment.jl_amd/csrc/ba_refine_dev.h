// Device pieces shared by the block refinements (ba_point_kernels.hip, ba_camera_kernels.hip).  Included inside
// the including file's unnamed namespace; gfx950 only.  Both files are built without FMA contraction: the operand order and the
// parentheses here are those of the model's device functions and must stay.
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
