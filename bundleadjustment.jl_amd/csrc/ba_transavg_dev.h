// Device pieces of translation averaging (ba_transavg_kernels.hip): unit vectors and symmetric 3 x 3 matrices as
// scalars in registers.  Included inside the including file's unnamed namespace; gfx950 only; built without FMA contraction.
// A vector is a double[3], a symmetric matrix a double[6] in the order (00, 01, 02, 11, 12, 22); both are only ever indexed by
// constants and only passed to functions that are forced inline, so they live in registers (an array indexed by a variable
// would go to scratch: tests/test_code_objects.py).
#pragma once

__device__ __forceinline__ double vec3_dot(const double x[3], const double y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__device__ __forceinline__ void vec3_cross(const double x[3], const double y[3], double z[3]) {
  z[0] = x[1] * y[2] - x[2] * y[1], z[1] = x[2] * y[0] - x[0] * y[2], z[2] = x[0] * y[1] - x[1] * y[0];
}

__device__ __forceinline__ double vec3_norm(const double x[3]) { return sqrt(vec3_dot(x, x)); }

// the angle between two vectors: atan2(|x x y|, x . y)
__device__ __forceinline__ double vec3_angle(const double x[3], const double y[3]) {
  double z[3];
  vec3_cross(x, y, z);
  return atan2(vec3_norm(z), vec3_dot(x, y));
}

// v <- sign * the three doubles at g
__device__ __forceinline__ void vec3_load(const double *__restrict__ g, bool negate, double v[3]) {
  const double a = g[0], b = g[1], c = g[2];
  v[0] = negate ? -a : a, v[1] = negate ? -b : b, v[2] = negate ? -c : c;
}

// The angular distance of the unit vector d to the shorter great-circle arc from the unit vector d1 to the unit vector d2
// (include/ba_hip.h, ba_translation_loops).  false: the arc is not defined (d1 and d2 opposite within 1e-6) and *e is untouched.
__device__ __forceinline__ bool arc_distance(const double d[3], const double d1[3], const double d2[3], double *e) {
  double n[3];
  vec3_cross(d1, d2, n);
  const double nn = vec3_norm(n);
  if (nn < 1e-6) {
    if (!(vec3_dot(d1, d2) > 0.0)) return false;
    *e = vec3_angle(d, d1);
    return true;
  }
  n[0] = n[0] / nn, n[1] = n[1] / nn, n[2] = n[2] / nn;
  const double h = vec3_dot(d, n);
  double q[3], s[3], t[3];
  q[0] = d[0] - h * n[0], q[1] = d[1] - h * n[1], q[2] = d[2] - h * n[2];
  vec3_cross(d1, q, s);
  vec3_cross(q, d2, t);
  if (vec3_dot(s, n) >= 0.0 && vec3_dot(t, n) >= 0.0) {
    *e = asin(fmin(1.0, fabs(h)));
  } else {
    *e = fmin(vec3_angle(d, d1), vec3_angle(d, d2));
  }
  return true;
}

// y <- S x, S symmetric
__device__ __forceinline__ void sym3_mul(const double S[6], const double x[3], double y[3]) {
  y[0] = (S[0] * x[0] + S[1] * x[1]) + S[2] * x[2];
  y[1] = (S[1] * x[0] + S[3] * x[1]) + S[4] * x[2];
  y[2] = (S[2] * x[0] + S[4] * x[1]) + S[5] * x[2];
}

// V <- the inverse of the symmetric S by cofactors.  false (and V = 0): det S is not above 1e-12 (tr S)^3 -- the determinant of
// a positive definite matrix is at most (tr / 3)^3, so this is a relative test; it also catches NaN.
__device__ __forceinline__ bool sym3_inverse(const double S[6], double V[6]) {
  const double c00 = S[3] * S[5] - S[4] * S[4], c01 = S[2] * S[4] - S[1] * S[5], c02 = S[1] * S[4] - S[2] * S[3];
  const double det = (S[0] * c00 + S[1] * c01) + S[2] * c02;
  const double tr = (S[0] + S[3]) + S[5];
  if (!(det > 1e-12 * ((tr * tr) * tr))) {
    V[0] = 0.0, V[1] = 0.0, V[2] = 0.0, V[3] = 0.0, V[4] = 0.0, V[5] = 0.0;
    return false;
  }
  V[0] = c00 / det, V[1] = c01 / det, V[2] = c02 / det;
  V[3] = (S[0] * S[5] - S[2] * S[2]) / det, V[4] = (S[1] * S[2] - S[0] * S[4]) / det, V[5] = (S[0] * S[3] - S[1] * S[1]) / det;
  return true;
}
