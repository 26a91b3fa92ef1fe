// Points with the cameras held (ba_refine_points): linear triangulation and a per-point Marquardt iteration on the
// handle's objective restricted to one point.  gfx950 only.
//
// With every camera entry of x held, point i is an independent problem in 3 unknowns:
//   f_i(X) = sum_{o in obs(i)} 1/2 c^2 rho(r^_o' r^_o / c^2) + 1/2 (X - mu)' Lambda (X - mu)
// (rho, c: ba_lm_set_loss; r^ = L'r: ba_lm_set_obs_info; the last term for a point with a point prior).  ONE launch runs the whole
// refinement: the iteration loop is inside k_refine_points, and the camera rows (cam_pre, 128 bytes per camera, L2-resident)
// come from k_cam_pre, launched once before it.  The residual and the point columns of the Jacobian are the model's own device
// functions (ba_model_dev.h): jac_block is inlined and only its columns 0..2 are used, so the 3 x 3 block G = d(P1)/dr and
// everything else of the camera columns is never computed.
//
// Two tiers by point degree (PT_TIER): a point of degree <= PT_TIER is one lane's work -- the lane walks pt_ptr / pt_obs with H, g
// and X in registers; a point of degree > PT_TIER gets one wave, whose lanes stride over the observations and sum their parts
// with an xor butterfly (every lane ends with the same bits, the wave then runs the 3 x 3 algebra uniformly).  A point is always
// in the same tier and its sums have a fixed order, so the result of a point depends on nothing but its own data.  No
// floating-point atomics; the eight counters of a call (states, BEHIND flags, most trials) are integers, added per workgroup.
//
// What this file has in common with ba_camera_kernels.hip is written once: the device pieces in ba_refine_dev.h, the host side
// (argument check, prior lookup, counter read-back, the body of the host-pointer entry; BlockWork) in ba_internal.h / ba_api.hip.
//
// ba_ransac_points puts a consensus stage in front: k_ransac_points, further down, finds every point's inlier set in
// one launch, k_ransac_mask_info (ba_ransac_kernels.hip) turns the set into information and k_refine_points runs unchanged on it.
#include <algorithm>
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

#include "ba_model_dev.h"  // CPAD, project_pre, jac_block
#include "ba_refine_dev.h"  // wave_all_sum, p1_z, UNDIST_ITERS
#include "ba_consensus_dev.h"  // sample_position: the draws of k_ransac_points are those of the camera side

constexpr int PT_BLK = 256;
// Degree above which a point gets a wave.  The lanes of a wave wait for its slowest lane, whose time grows with degree x trials:
// 32 bounds a lane's serial chain per evaluation at 32 observations, and a point above it keeps at least half of the lanes of its
// own wave busy.  The lane tier's points are ordered by descending degree, so the lanes of one wave walk lists of similar length.
constexpr int PT_TIER = 32;

struct PtArgs {
  const int *pt_ptr, *pt_obs, *cam0;
  const double *pt2d, *cpre, *info;  // info: l00 l10 l11 per observation, or null
  const uint8_t *fixed;              // or null
  const int *pri_of;                 // point -> its point prior, -1: none; or null
  const double *pri_mu, *pri_info;
  const int *lane_pts, *wave_pts;
  int n_lane, n_wave;
  double *x;
  uint8_t *status;  // or null
  double *cost;     // or null
  unsigned long long *counts;
  int init, max_iter, kind;
  double xtol, lambda0, c2;
};

// A x = b by Cholesky, A symmetric 3 x 3 packed lower row-major (xx xy yy xz yz zz).  False when a pivot is not above piv_min or
// the solution is not finite.
__device__ __forceinline__ bool chol3_solve(const double A[6], const double b[3], double piv_min, double x[3]) {
  const double d0 = A[0];
  if (!(d0 > piv_min)) return false;
  const double l00 = sqrt(d0), l10 = A[1] / l00, l20 = A[3] / l00;
  const double d1 = A[2] - l10 * l10;
  if (!(d1 > piv_min)) return false;
  const double l11 = sqrt(d1), l21 = (A[4] - l20 * l10) / l11;
  const double d2 = A[5] - l20 * l20 - l21 * l21;
  if (!(d2 > piv_min)) return false;
  const double l22 = sqrt(d2);
  const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
  return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// observation k of a point's list: its cam_pre row, its measurement and its information factors
struct PtObs {
  double P[12];
  double mx, my, l00, l10, l11;
  bool used;  // Lambda != 0
};
__device__ __forceinline__ void load_obs(const PtArgs &a, int k, PtObs &ob) {
  const int o = a.pt_obs[k];
  const double2 *row = reinterpret_cast<const double2 *>(a.cpre + CPAD * (int64_t)a.cam0[o]);
#pragma unroll
  for (int u = 0; u < 6; u++) {
    const double2 v = row[u];
    ob.P[2 * u] = v.x;
    ob.P[2 * u + 1] = v.y;
  }
  const double2 m = reinterpret_cast<const double2 *>(a.pt2d)[o];
  ob.mx = m.x;
  ob.my = m.y;
  ob.l00 = 1.0, ob.l10 = 0.0, ob.l11 = 1.0;
  if (a.info) ob.l00 = a.info[3 * (int64_t)o], ob.l10 = a.info[3 * (int64_t)o + 1], ob.l11 = a.info[3 * (int64_t)o + 2];
  ob.used = !(ob.l00 == 0.0 && ob.l10 == 0.0 && ob.l11 == 0.0);
}

// f, H = sum w J^'J^ (+ Lambda), g = sum w J^'r^ (+ Lambda (X - mu)) of one point at X, and whether an observation with
// Lambda != 0 has P1.z >= 0 there
template <bool WAVE>
__device__ __forceinline__ void point_eval(const PtArgs &a, int k0, int k1, int lane, const double X[3], bool prior, const double mu[3],
                                           const double Lm[6], double &f, double H[6], double g[3], int &behind) {
  double fs = 0.0, hs[6] = {0, 0, 0, 0, 0, 0}, gs[3] = {0, 0, 0};
  int bh = 0;
  for (int k = k0 + (WAVE ? lane : 0); k < k1; k += (WAVE ? 64 : 1)) {
    PtObs ob;
    load_obs(a, k, ob);
    double out[2], J[24];
    project_pre<double>(X, ob.P, out);
    jac_block<double>(X, ob.P, J);  // (columns 0..2 of both rows are used: G and the intrinsics' columns are dead code)
    double z1;
    p1_z(ob.P, X, z1);
    if (ob.used && z1 >= 0.0) bh = 1;
    const double ex = out[0] - ob.mx, ey = out[1] - ob.my;
    const double rx = ob.l00 * ex + ob.l10 * ey, ry = ob.l11 * ey;
    double j0[3], j1[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      j0[i] = ob.l00 * J[i] + ob.l10 * J[12 + i];
      j1[i] = ob.l11 * J[12 + i];
    }
    double w;
    fs += robust_rho(a.kind, rx * rx + ry * ry, a.c2, &w);
    hs[0] += w * (j0[0] * j0[0] + j1[0] * j1[0]);
    hs[1] += w * (j0[1] * j0[0] + j1[1] * j1[0]);
    hs[2] += w * (j0[1] * j0[1] + j1[1] * j1[1]);
    hs[3] += w * (j0[2] * j0[0] + j1[2] * j1[0]);
    hs[4] += w * (j0[2] * j0[1] + j1[2] * j1[1]);
    hs[5] += w * (j0[2] * j0[2] + j1[2] * j1[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) gs[i] += w * (j0[i] * rx + j1[i] * ry);
  }
  if (WAVE) {
    fs = wave_all_sum(fs);
#pragma unroll
    for (int i = 0; i < 6; i++) hs[i] = wave_all_sum(hs[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) gs[i] = wave_all_sum(gs[i]);
    bh = __any(bh) ? 1 : 0;
  }
  f = 0.5 * fs;
  if (prior) {
    const double d[3] = {X[0] - mu[0], X[1] - mu[1], X[2] - mu[2]};
    const double q[3] = {Lm[0] * d[0] + Lm[1] * d[1] + Lm[3] * d[2], Lm[1] * d[0] + Lm[2] * d[1] + Lm[4] * d[2],
                         Lm[3] * d[0] + Lm[4] * d[1] + Lm[5] * d[2]};
    f += 0.5 * (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]);
#pragma unroll
    for (int i = 0; i < 6; i++) hs[i] += Lm[i];
#pragma unroll
    for (int i = 0; i < 3; i++) gs[i] += q[i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) H[i] = hs[i];
#pragma unroll
  for (int i = 0; i < 3; i++) g[i] = gs[i];
  behind = bh;
}

// Linear triangulation: the point nearest to the rays of its observations with Lambda != 0.  Per observation the measurement is
// undistorted (u = pt2d / f, q <- u / (1 + k1 |q|^2 + k2 |q|^4)), the ray is d = R'(q_x, q_y, -1) / |.| through the centre
// c = -R't, and X solves sum (I - dd') X = sum (I - dd') c.  False: fewer than two such observations, or a pivot <= 1e-12 trace.
template <bool WAVE>
__device__ __forceinline__ bool point_triangulate(const PtArgs &a, int k0, int k1, int lane, double X[3]) {
  double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, n = 0.0;
  for (int k = k0 + (WAVE ? lane : 0); k < k1; k += (WAVE ? 64 : 1)) {
    PtObs ob;
    load_obs(a, k, ob);
    if (!ob.used) continue;
    const double kx = ob.P[0], ky = ob.P[1], kz = ob.P[2], s = ob.P[9], c = ob.P[10];
    const double ux = ob.mx / ob.P[8], uy = ob.my / ob.P[8];
    double qx = ux, qy = uy;
#pragma unroll
    for (int it = 0; it < UNDIST_ITERS; it++) {
      const double n2 = qx * qx + qy * qy;
      const double sc = 1.0 + ob.P[6] * n2 + ob.P[7] * (n2 * n2);
      qx = ux / sc;
      qy = uy / sc;
    }
    // R'v = cos v - sin (k x v) + (1 - cos) (k . v) k
    const double v[3] = {qx, qy, -1.0}, t[3] = {ob.P[3], ob.P[4], ob.P[5]}, kk[3] = {kx, ky, kz};
    const double kv = kx * v[0] + ky * v[1] + kz * v[2], kt = kx * t[0] + ky * t[1] + kz * t[2];
    const double xv[3] = {ky * v[2] - kz * v[1], kz * v[0] - kx * v[2], kx * v[1] - ky * v[0]};
    const double xt[3] = {ky * t[2] - kz * t[1], kz * t[0] - kx * t[2], kx * t[1] - ky * t[0]};
    double d[3], cc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      d[i] = c * v[i] - s * xv[i] + (1 - c) * kv * kk[i];
      cc[i] = -(c * t[i] - s * xt[i] + (1 - c) * kt * kk[i]);
    }
    const double inv = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] *= inv;
    const double dc = d[0] * cc[0] + d[1] * cc[1] + d[2] * cc[2];
    A[0] += 1.0 - d[0] * d[0];
    A[1] += -d[1] * d[0];
    A[2] += 1.0 - d[1] * d[1];
    A[3] += -d[2] * d[0];
    A[4] += -d[2] * d[1];
    A[5] += 1.0 - d[2] * d[2];
#pragma unroll
    for (int i = 0; i < 3; i++) b[i] += cc[i] - d[i] * dc;
    n += 1.0;
  }
  if (WAVE) {
#pragma unroll
    for (int i = 0; i < 6; i++) A[i] = wave_all_sum(A[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) b[i] = wave_all_sum(b[i]);
    n = wave_all_sum(n);
  }
  if (n < 2.0) return false;
  return chol3_solve(A, b, 1e-12 * (A[0] + A[2] + A[5]), X);
}

// One point: lane tier -- this lane alone; wave tier -- all 64 lanes of the wave together (the control flow is wave-uniform)
template <bool WAVE>
__device__ __forceinline__ void refine_point(const PtArgs &a, int i, int lane, int &status_out, int &trials_out) {
  const int k0 = a.pt_ptr[i], k1 = a.pt_ptr[i + 1];
  double *xp = a.x + 3 * (int64_t)i;
  const bool fixed = a.fixed != nullptr && a.fixed[i] != 0;
  const int q = a.pri_of ? a.pri_of[i] : -1;
  const bool prior = q >= 0;
  double mu[3] = {0, 0, 0}, Lm[6] = {0, 0, 0, 0, 0, 0};
  if (prior) {
#pragma unroll
    for (int j = 0; j < 3; j++) mu[j] = a.pri_mu[3 * (int64_t)q + j];
#pragma unroll
    for (int j = 0; j < 6; j++) Lm[j] = a.pri_info[6 * (int64_t)q + j];
  }
  int status = BA_PT_DEGENERATE, trials = 0, behind = 0;
  double fb = 0.0, fa = 0.0, X[3] = {0, 0, 0};
  bool write = false;
  if (fixed || k1 > k0) {  // (a free point without an observation: DEGENERATE, untouched)
    bool have = true;
    if (a.init == 1 && !fixed) {
      have = point_triangulate<WAVE>(a, k0, k1, lane, X);
      write = have;
    } else {
      X[0] = xp[0], X[1] = xp[1], X[2] = xp[2];
    }
    if (have) {
      double f, H[6], g[3];
      point_eval<WAVE>(a, k0, k1, lane, X, prior, mu, Lm, f, H, g, behind);
      fb = fa = f;
      if (fixed) {
        status = BA_PT_FIXED;
      } else if (!isfinite(f)) {
        status = BA_PT_NONFINITE;
        write = false;
        behind = 0;
      } else {
        status = BA_PT_MAX_ITER;
        double lam = a.lambda0;
        for (int it = 0; it < a.max_iter; it++) {
          trials = it + 1;
          const double A[6] = {H[0] + lam * H[0], H[1], H[2] + lam * H[2], H[3], H[4], H[5] + lam * H[5]};
          const double nb[3] = {-g[0], -g[1], -g[2]};
          double d[3], Xn[3], fn = 0.0, Hn[6], gn[3];
          int bn = 0;
          bool accept = false;
          if (chol3_solve(A, nb, 0.0, d)) {
            Xn[0] = X[0] + d[0], Xn[1] = X[1] + d[1], Xn[2] = X[2] + d[2];
            point_eval<WAVE>(a, k0, k1, lane, Xn, prior, mu, Lm, fn, Hn, gn, bn);
            accept = fn <= f;  // (false for a NaN)
          }
          if (accept) {
            X[0] = Xn[0], X[1] = Xn[1], X[2] = Xn[2];
            f = fn;
#pragma unroll
            for (int j = 0; j < 6; j++) H[j] = Hn[j];
#pragma unroll
            for (int j = 0; j < 3; j++) g[j] = gn[j];
            behind = bn;
            write = true;
            lam = fmax(lam / 10.0, 1e-12);
            const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const double nx = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
            if (nd <= a.xtol * (nx + a.xtol)) {
              status = BA_PT_CONVERGED;
              break;
            }
          } else {
            lam *= 10.0;
            if (lam > 1e12) {
              status = BA_PT_STALLED;
              break;
            }
          }
        }
        fa = f;
      }
    }
  }
  if (!WAVE || lane == 0) {
    if (write) xp[0] = X[0], xp[1] = X[1], xp[2] = X[2];
    if (a.status) a.status[i] = (uint8_t)(status | (behind ? BA_PT_BEHIND : 0));
    if (a.cost) a.cost[2 * (int64_t)i] = fb, a.cost[2 * (int64_t)i + 1] = fa;
  }
  status_out = status | (behind ? BA_PT_BEHIND : 0);
  trials_out = trials;
}

// ---- the consensus stage of ba_ransac_points (include/ba_hip.h, "outlier-robust triangulation") ---------------------
// k_ransac_points, in the grid of k_refine_points: hypotheses, selection, marking and refits of a point in ONE launch.  The
// camera side (ba_ransac_kernels.hip) has a few thousand long lists and gives every hypothesis a wave and a slot of a table in
// global memory; here there are a million short lists, a table would be npnts x H ints, and a hypothesis is a 3 x 3 solve on two
// rays: the running best (count, h, X) of a list stays in registers and nothing per hypothesis is stored.
//   lane tier   the lane runs its point's hypotheses one after the other; its set is a 32-bit mask in a register (d <= PT_TIER)
//               and the inlier bytes are written once, at the end.
//   wave tier   the 64 lanes take 64 hypotheses at a time: each lane triangulates its own pair, then all lanes walk the point's
//               list in lockstep -- every lane loads the same camera row and the same measurement -- and count under their own X.
//               One max-reduction over the key of consensus_winner (count above inverted h) picks the winner and its X comes
//               from its lane by shuffle.  The refits are the wave-strided triangulation and a strided re-score, the set in the
//               inlier bytes with bit 1 carrying M' between the two passes (the rule of consensus_rescore, at wave scope: every
//               lane rewrites the bytes it wrote).
// The sampling is that of the camera side (sample_position: the same key and draws) with the skip rule and the 64-draw limit of
// sample_take run by one lane, since a lane owns a hypothesis here.  Integer results only cross lanes; every output has one
// writer; no LDS.  The finish is k_refine_points itself on the masked information (k_ransac_mask_info).
struct PtConsensus {
  uint8_t *inlier;            // nobs
  int *n_inliers, *best_hyp;  // npnts
  int hypotheses, min_inliers, refits;
  uint64_t seed_mix;  // mix(seed)
  double tau2;
};

// What one observation adds to the sums of the linear triangulation: a copy of the loop body of point_triangulate, which stays
// as it is (k_refine_points is the finish and keeps its code).
__device__ __forceinline__ void ray_terms(const PtObs &ob, double A[6], double b[3]) {
  const double kx = ob.P[0], ky = ob.P[1], kz = ob.P[2], s = ob.P[9], c = ob.P[10];
  const double ux = ob.mx / ob.P[8], uy = ob.my / ob.P[8];
  double qx = ux, qy = uy;
#pragma unroll
  for (int it = 0; it < UNDIST_ITERS; it++) {
    const double n2 = qx * qx + qy * qy;
    const double sc = 1.0 + ob.P[6] * n2 + ob.P[7] * (n2 * n2);
    qx = ux / sc;
    qy = uy / sc;
  }
  const double v[3] = {qx, qy, -1.0}, t[3] = {ob.P[3], ob.P[4], ob.P[5]}, kk[3] = {kx, ky, kz};
  const double kv = kx * v[0] + ky * v[1] + kz * v[2], kt = kx * t[0] + ky * t[1] + kz * t[2];
  const double xv[3] = {ky * v[2] - kz * v[1], kz * v[0] - kx * v[2], kx * v[1] - ky * v[0]};
  const double xt[3] = {ky * t[2] - kz * t[1], kz * t[0] - kx * t[2], kx * t[1] - ky * t[0]};
  double d[3], cc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    d[i] = c * v[i] - s * xv[i] + (1 - c) * kv * kk[i];
    cc[i] = -(c * t[i] - s * xt[i] + (1 - c) * kt * kk[i]);
  }
  const double inv = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
  for (int i = 0; i < 3; i++) d[i] *= inv;
  const double dc = d[0] * cc[0] + d[1] * cc[1] + d[2] * cc[2];
  A[0] = 1.0 - d[0] * d[0];
  A[1] = -d[1] * d[0];
  A[2] = 1.0 - d[1] * d[1];
  A[3] = -d[2] * d[0];
  A[4] = -d[2] * d[1];
  A[5] = 1.0 - d[2] * d[2];
#pragma unroll
  for (int i = 0; i < 3; i++) b[i] = cc[i] - d[i] * dc;
}

// the linear triangulation on the entries of [k0, k1) that are used and that pick(k) keeps: the sums and the solve of
// point_triangulate
template <bool WAVE, typename Pick>
__device__ __forceinline__ bool triangulate_picked(const PtArgs &a, int k0, int k1, int lane, Pick pick, double X[3]) {
  double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, n = 0.0;
  for (int k = k0 + (WAVE ? lane : 0); k < k1; k += (WAVE ? 64 : 1)) {
    PtObs ob;
    load_obs(a, k, ob);
    if (!ob.used || !pick(k)) continue;
    double At[6], bt[3];
    ray_terms(ob, At, bt);
#pragma unroll
    for (int i = 0; i < 6; i++) A[i] += At[i];
#pragma unroll
    for (int i = 0; i < 3; i++) b[i] += bt[i];
    n += 1.0;
  }
  if (WAVE) {
#pragma unroll
    for (int i = 0; i < 6; i++) A[i] = wave_all_sum(A[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) b[i] = wave_all_sum(b[i]);
    n = wave_all_sum(n);
  }
  if (n < 2.0) return false;
  return chol3_solve(A, b, 1e-12 * (A[0] + A[2] + A[5]), X);
}

// the inlier test of the header under the point X: used, in front (P1.z < 0), within tau of its measurement in raw pixels (a
// comparison with NaN fails)
__device__ __forceinline__ bool point_inlier(const PtObs &ob, const double X[3], double tau2) {
  double out[2], z1;
  project_pre<double>(X, ob.P, out);
  p1_z(ob.P, X, z1);
  const double ex = out[0] - ob.mx, ey = out[1] - ob.my;
  return ob.used && z1 < 0.0 && ex * ex + ey * ey <= tau2;
}

// the pair (pa < pb) of rank h < d (d - 1) / 2 in the order (0,1), (0,2), ..., (0,d-1), (1,2), ...: row pa starts at rank
// pa (2 d - pa - 1) / 2; the square root gives the row within one, the two loops settle it
__device__ __forceinline__ void pair_unrank(int h, int d, int &pa, int &pb) {
  const double s = 2.0 * d - 1.0;
  int r = (int)((s - sqrt(fmax(s * s - 8.0 * h, 0.0))) * 0.5);
  r = r < 0 ? 0 : (r > d - 2 ? d - 2 : r);
  while (r < d - 2 && (r + 1) * (2 * d - r - 2) / 2 <= h) r++;
  while (r > 0 && r * (2 * d - r - 1) / 2 > h) r--;
  pa = r;
  pb = r + 1 + (h - r * (2 * d - r - 1) / 2);
}

// The sample of hypothesis h in a list of d entries, m = 2, by one lane: draw j = 0, 1, ... of sample_position; a draw is skipped
// when its entry is not used or an earlier draw hit its position; the first two that count are the sample; fewer after RN_DRAWS
// draws: void.
__device__ __forceinline__ bool sample_pair(const PtArgs &a, uint64_t seed_mix, int h, int k0, int d, int &pa, int &pb) {
  int n = 0;
  pa = pb = -1;
  for (int j = 0; j < RN_DRAWS && n < 2; j++) {
    const int pos = sample_position(seed_mix, h, j, d);
    if (pos == pa || !obs_used(a.info, a.pt_obs[k0 + pos])) continue;
    if (n == 0) pa = pos;
    else pb = pos;
    n++;
  }
  return n == 2;
}

// Hypothesis h of the list [k0, k0 + d): its two list positions (exhaustive: the pair of rank h; otherwise the sample) and the
// linear triangulation on them; false: void.  next: the exhaustive enumeration advances (pa, pb) from the pair of rank h - 1
// instead of unranking (the lane tier walks h in order).
template <bool NEXT>
__device__ __forceinline__ bool hypothesis_point(const PtArgs &a, const PtConsensus &c, bool exhaustive, int h, int k0, int d, int &pa,
                                                 int &pb, double X[3]) {
  if (exhaustive) {
    if (NEXT) {
      if (++pb >= d) pa++, pb = pa + 1;
    } else {
      pair_unrank(h, d, pa, pb);
    }
  } else if (!sample_pair(a, c.seed_mix, h, k0, d, pa, pb)) {
    return false;
  }
  PtObs oa, ob;
  load_obs(a, k0 + pa, oa);
  load_obs(a, k0 + pb, ob);
  if (!oa.used || !ob.used) return false;
  double A[6], b[3], At[6], bt[3];
  ray_terms(oa, A, b);
  ray_terms(ob, At, bt);
#pragma unroll
  for (int i = 0; i < 6; i++) A[i] += At[i];
#pragma unroll
  for (int i = 0; i < 3; i++) b[i] += bt[i];
  return chol3_solve(A, b, 1e-12 * (A[0] + A[2] + A[5]), X);
}

// a point that is not attempted: its set is its used observations
template <bool WAVE>
__device__ __forceinline__ void consensus_skip(const PtArgs &a, const PtConsensus &c, int i, int k0, int k1, int lane) {
  int n = 0;
  for (int k = k0 + (WAVE ? lane : 0); k < k1; k += (WAVE ? 64 : 1)) {
    const int o = a.pt_obs[k];
    const int u = obs_used(a.info, o) ? 1 : 0;
    c.inlier[o] = (uint8_t)u;
    n += u;
  }
  if (WAVE) n = wave_all_sum_int(n);
  if (!WAVE || lane == 0) c.n_inliers[i] = n, c.best_hyp[i] = -1;
}

// lane tier: one point per lane, d <= PT_TIER
__device__ __forceinline__ void consensus_point_lane(const PtArgs &a, const PtConsensus &c, int i) {
  static_assert(PT_TIER <= 32, "the set of a lane-tier point is a 32-bit mask");
  const int k0 = a.pt_ptr[i], k1 = a.pt_ptr[i + 1], d = k1 - k0;
  if (a.fixed != nullptr && a.fixed[i] != 0) {
    consensus_skip<false>(a, c, i, k0, k1, 0);
    return;
  }
  const int npairs = d * (d - 1) / 2;
  const bool exhaustive = npairs <= c.hypotheses;
  const int nh = exhaustive ? npairs : c.hypotheses;
  int best = -1, best_count = -1, pa = 0, pb = 0;
  double Xb[3] = {0, 0, 0};
  for (int h = 0; h < nh; h++) {
    double X[3];
    if (!hypothesis_point<true>(a, c, exhaustive, h, k0, d, pa, pb, X)) continue;
    int cnt = 0;
    for (int k = k0; k < k1; k++) {
      PtObs ob;
      load_obs(a, k, ob);
      cnt += point_inlier(ob, X, c.tau2) ? 1 : 0;
    }
    if (cnt > best_count) {  // (h ascends: a tie stays with the lower h)
      best = h, best_count = cnt;
      Xb[0] = X[0], Xb[1] = X[1], Xb[2] = X[2];
    }
  }
  unsigned M = 0;
  int n = best_count < 0 ? 0 : best_count;
  if (best >= 0 && best_count >= c.min_inliers) {
    for (int k = k0; k < k1; k++) {
      PtObs ob;
      load_obs(a, k, ob);
      if (point_inlier(ob, Xb, c.tau2)) M |= 1u << (k - k0);
    }
    for (int r = 0; r < c.refits; r++) {
      double Xn[3];
      if (!triangulate_picked<false>(a, k0, k1, 0, [&](int k) { return ((M >> (k - k0)) & 1u) != 0; }, Xn)) break;
      unsigned M2 = 0;
      for (int k = k0; k < k1; k++) {
        PtObs ob;
        load_obs(a, k, ob);
        if (point_inlier(ob, Xn, c.tau2)) M2 |= 1u << (k - k0);
      }
      const int n2 = __popc(M2);
      if (n2 < n || M2 == M) break;
      M = M2, n = n2;
    }
  }
  for (int k = k0; k < k1; k++) c.inlier[a.pt_obs[k]] = (uint8_t)((M >> (k - k0)) & 1u);
  c.n_inliers[i] = n, c.best_hyp[i] = best;
}

// wave tier: one point per wave (the control flow is wave-uniform)
__device__ __forceinline__ void consensus_point_wave(const PtArgs &a, const PtConsensus &c, int i, int lane) {
  static_assert(RN_HYP_MAX == 1 << 12, "the selection key holds h in 12 bits");
  const int k0 = a.pt_ptr[i], k1 = a.pt_ptr[i + 1], d = k1 - k0;
  if (a.fixed != nullptr && a.fixed[i] != 0) {
    consensus_skip<true>(a, c, i, k0, k1, lane);
    return;
  }
  const long long npairs = (long long)d * (d - 1) / 2;
  const bool exhaustive = npairs <= (long long)c.hypotheses;
  const int nh = exhaustive ? (int)npairs : c.hypotheses;
  long long key = 0;  // this lane's best: count + 1 above the inverted h (consensus_winner), 0: none
  double Xb[3] = {0, 0, 0};
  for (int base = 0; base < nh; base += 64) {
    const int h = base + lane;
    int pa = 0, pb = 0;
    double X[3] = {0, 0, 0};
    const bool ok = h < nh && hypothesis_point<false>(a, c, exhaustive, h, k0, d, pa, pb, X);
    if (!__any(ok)) continue;
    int cnt = 0;
    for (int k = k0; k < k1; k++) {  // (the same entry in every lane)
      PtObs ob;
      load_obs(a, k, ob);
      cnt += point_inlier(ob, X, c.tau2) ? 1 : 0;
    }
    const long long kk = ((long long)(cnt + 1) << 12) | (long long)(4095 - h);
    if (ok && kk > key) {
      key = kk;
      Xb[0] = X[0], Xb[1] = X[1], Xb[2] = X[2];
    }
  }
  long long top = key;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long other = __shfl_xor(top, off, 64);
    top = other > top ? other : top;
  }
  const int best = top ? 4095 - (int)(top & 4095) : -1, best_count = top ? (int)(top >> 12) - 1 : 0;
  if (best < 0 || best_count < c.min_inliers) {
    for (int k = k0 + lane; k < k1; k += 64) c.inlier[a.pt_obs[k]] = 0;
    if (lane == 0) c.n_inliers[i] = best_count, c.best_hyp[i] = best;
    return;
  }
  const int src = __ffsll((long long)__ballot(key == top)) - 1;  // (the keys of two lanes differ in h: one lane)
  double Xw[3] = {__shfl(Xb[0], src, 64), __shfl(Xb[1], src, 64), __shfl(Xb[2], src, 64)};
  int n = 0;
  for (int k = k0 + lane; k < k1; k += 64) {
    PtObs ob;
    load_obs(a, k, ob);
    const int in = point_inlier(ob, Xw, c.tau2) ? 1 : 0;
    c.inlier[a.pt_obs[k]] = (uint8_t)in;
    n += in;
  }
  n = wave_all_sum_int(n);
  for (int r = 0; r < c.refits; r++) {
    double Xn[3];
    if (!triangulate_picked<true>(a, k0, k1, lane, [&](int k) { return (c.inlier[a.pt_obs[k]] & 1) != 0; }, Xn)) break;
    int n2 = 0, diff = 0;
    for (int k = k0 + lane; k < k1; k += 64) {
      PtObs ob;
      load_obs(a, k, ob);
      const int o = a.pt_obs[k];
      const int in = point_inlier(ob, Xn, c.tau2) ? 1 : 0, old = c.inlier[o] & 1;
      c.inlier[o] = (uint8_t)(old | (in << 1));
      n2 += in;
      diff += in != old ? 1 : 0;
    }
    n2 = wave_all_sum_int(n2);
    diff = wave_all_sum_int(diff);
    const bool adopt = n2 >= n && diff > 0;
    for (int k = k0 + lane; k < k1; k += 64) {
      const int o = a.pt_obs[k];
      const int b = c.inlier[o];
      c.inlier[o] = (uint8_t)(adopt ? (b >> 1) & 1 : b & 1);
    }
    if (!adopt) break;
    n = n2;
  }
  if (lane == 0) c.n_inliers[i] = n, c.best_hyp[i] = best;
}

// the grid of k_refine_points: the wave tier's workgroups first
__global__ __launch_bounds__(PT_BLK) void k_ransac_points(PtArgs a, PtConsensus c) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nb_wave = (a.n_wave + PT_BLK / 64 - 1) / (PT_BLK / 64);
  if ((int)blockIdx.x < nb_wave) {
    const int idx = (int)blockIdx.x * (PT_BLK / 64) + wv;  // (wave-uniform)
    if (idx < a.n_wave) consensus_point_wave(a, c, a.wave_pts[idx], lane);
  } else {
    const int64_t idx = (int64_t)((int)blockIdx.x - nb_wave) * PT_BLK + t;
    if (idx < a.n_lane) consensus_point_lane(a, c, a.lane_pts[idx]);
  }
}

// (k_ransac_points stands in front of k_refine_points in this file so that the latter stays the last symbol of the code object,
// as it was: tools/compare_code_objects.py then shows it unchanged line for line.)
// Workgroups [0, ceil(n_wave / 4)): one point of wave_pts per wave (they run longest and start first); the others: one point of
// lane_pts per lane.
__global__ __launch_bounds__(PT_BLK) void k_refine_points(PtArgs a) {
  __shared__ unsigned cnt[BLOCK_COUNTERS];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < BLOCK_COUNTERS) cnt[t] = 0;
  __syncthreads();
  const int nb_wave = (a.n_wave + PT_BLK / 64 - 1) / (PT_BLK / 64);
  int status = -1, trials = 0;
  if ((int)blockIdx.x < nb_wave) {
    const int idx = (int)blockIdx.x * (PT_BLK / 64) + wv;  // (wave-uniform)
    if (idx < a.n_wave) {
      refine_point<true>(a, a.wave_pts[idx], lane, status, trials);
      if (lane != 0) status = -1;
    }
  } else {
    const int64_t idx = (int64_t)((int)blockIdx.x - nb_wave) * PT_BLK + t;
    if (idx < a.n_lane) refine_point<false>(a, a.lane_pts[idx], lane, status, trials);
  }
  if (status >= 0) {
    atomicAdd(&cnt[status & 0x7f], 1u);
    if (status & BA_PT_BEHIND) atomicAdd(&cnt[BA_PT_STATES], 1u);
    atomicMax(&cnt[BA_PT_STATES + 1], (unsigned)trials);
  }
  __syncthreads();
  if (t < BLOCK_COUNTERS && cnt[t] != 0) {
    if (t == BA_PT_STATES + 1) atomicMax(a.counts + t, (unsigned long long)cnt[t]);
    else atomicAdd(a.counts + t, (unsigned long long)cnt[t]);
  }
}

}  // namespace

// the point list split by degree (once per problem) and the lookup of the point priors (once per ba_lm_set_priors)
static int point_tables(ba_problem *p) {
  PointWork &w = p->pts;
  if (!w.split) {
    // counting sort by descending degree, stable: [degree > PT_TIER | PT_TIER .. 0]
    std::vector<int64_t> start((size_t)PT_TIER + 3, 0);
    auto bucket = [&](int64_t i) {
      const int deg = p->h_pt_ptr[(size_t)i + 1] - p->h_pt_ptr[(size_t)i];
      return deg > PT_TIER ? 0 : 1 + (PT_TIER - deg);
    };
    for (int64_t i = 0; i < p->npnts; i++) start[(size_t)bucket(i) + 1]++;
    for (size_t b = 1; b < start.size(); b++) start[b] += start[b - 1];
    const int64_t nw = start[1];
    std::vector<int> order((size_t)p->npnts);
    {
      std::vector<int64_t> at(start.begin(), start.end() - 1);
      for (int64_t i = 0; i < p->npnts; i++) order[(size_t)at[(size_t)bucket(i)]++] = (int)i;
    }
    // the wave tier's points by descending degree as well: the longest start first
    std::stable_sort(order.begin(), order.begin() + nw, [&](int u, int v) {
      return p->h_pt_ptr[(size_t)u + 1] - p->h_pt_ptr[(size_t)u] > p->h_pt_ptr[(size_t)v + 1] - p->h_pt_ptr[(size_t)v];
    });
    BA_CHECK(upload(w.wave_pts, std::vector<int>(order.begin(), order.begin() + nw)));
    BA_CHECK(upload(w.lane_pts, std::vector<int>(order.begin() + nw, order.end())));
    BA_CHECK(w.counts.alloc(BLOCK_COUNTERS));
    w.n_wave = nw;
    w.n_lane = p->npnts - nw;
    w.split = true;
  }
  if (w.pri_version != p->pri_version) {
    BA_CHECK(block_prior_lookup(p->pri[PRI_PNT], p->npnts, w.pri_of));
    w.pri_version = p->pri_version;
  }
  return BA_OK;
}

static int refine_check(const char *who, ba_problem *p, const double *x, int init, int *max_iter, double *xtol, double *lambda0) {
  return block_check(who, p, x, 50, max_iter, xtol, lambda0, [&] {
    if (init == 0 || init == 1) return BA_OK;
    ba_set_error("%s: init must be 0 (start from the points of x) or 1 (triangulate first), got %d", who, init);
    return BA_ERR_ARG;
  });
}

// (ransac: k_ransac_points and k_ransac_mask_info, which leave the set as information, then) k_refine_points on st, behind
// k_cam_pre; the counters stay on the device (p->pts.counts)
static int refine_launch(ba_problem *p, double *d_x, int init, const ba_ransac_opts *ransac, int max_iter, double xtol, double lambda0,
                         uint8_t *d_status, double *d_cost, hipStream_t st) {
  BA_CHECK(terms_upload(p));
  BA_CHECK(point_tables(p));
  PointWork &w = p->pts;
  BA_HIP_CHECK(hipMemsetAsync(w.counts, 0, BLOCK_COUNTERS * sizeof(unsigned long long), st));
  if (p->npnts == 0) return BA_OK;
  if (ransac && !w.rs_inlier) {
    BA_CHECK(w.rs_inlier.alloc(p->nobs));
    BA_CHECK(w.rs_info.alloc(3 * p->nobs));
    BA_CHECK(w.rs_n.alloc(p->npnts));
    BA_CHECK(w.rs_best.alloc(p->npnts));
  }
  const PriorSet &pt = p->pri[PRI_PNT];
  PtArgs a;
  a.pt_ptr = p->pt_ptr, a.pt_obs = p->pt_obs, a.cam0 = p->cam0;
  a.pt2d = p->pt2d, a.cpre = nullptr, a.info = p->info_on() ? (const double *)p->d_info : nullptr;
  a.fixed = p->fix_npnt > 0 ? (const uint8_t *)p->d_fix_pnt : nullptr;
  a.pri_of = pt.n > 0 ? (const int *)w.pri_of : nullptr;
  a.pri_mu = pt.n > 0 ? (const double *)pt.mu : nullptr, a.pri_info = pt.n > 0 ? (const double *)pt.info : nullptr;
  a.lane_pts = w.lane_pts, a.wave_pts = w.wave_pts;
  a.n_lane = (int)w.n_lane, a.n_wave = (int)w.n_wave;
  a.x = d_x, a.status = d_status, a.cost = d_cost, a.counts = w.counts;
  a.init = init, a.max_iter = max_iter, a.kind = p->loss;
  a.xtol = xtol, a.lambda0 = lambda0, a.c2 = p->loss_scale * p->loss_scale;
  const unsigned grid = grid_for(w.n_wave, PT_BLK / 64) + grid_for(w.n_lane, PT_BLK);
  if (ransac) {
    // the consensus stage: the set reaches k_refine_points as information -- w.rs_info, the masked copy of the factors (1 0 1
    // when the caller set none: the values the kernel uses without an array)
    ProfScope ps(p, PC_RANSAC_POINTS, st);
    BA_CHECK(launch_cam_pre_f64(p, d_x, &a.cpre, st));
    PtConsensus c;
    c.inlier = w.rs_inlier, c.n_inliers = w.rs_n, c.best_hyp = w.rs_best;
    c.hypotheses = ransac->hypotheses, c.min_inliers = ransac->min_inliers, c.refits = ransac->refits;
    c.seed_mix = ransac_seed_mix(ransac->seed), c.tau2 = ransac->threshold * ransac->threshold;
    BA_CHECK(BA_LAUNCH(k_ransac_points, grid, PT_BLK, 0, st, a, c));
    RansacArgs r = {};
    r.inlier = w.rs_inlier, r.info = a.info;
    BA_CHECK(launch_ransac_mask_info(r, p->nobs, w.rs_info, st));
    a.info = w.rs_info;
  }
  ProfScope ps(p, PC_REFINE_POINTS, st);
  if (!ransac) BA_CHECK(launch_cam_pre_f64(p, d_x, &a.cpre, st));  // (behind the consensus stage the rows are there)
  return BA_LAUNCH(k_refine_points, grid, PT_BLK, 0, st, a);
}

extern "C" int ba_refine_points_dev(ba_problem *p, double *d_x_inout, int init, int max_iter, double xtol, double lambda0,
                                    uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max, void *stream) {
  BA_CHECK(refine_check("ba_refine_points_dev", p, d_x_inout, init, &max_iter, &xtol, &lambda0));
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)p->stream;
  BA_CHECK(refine_launch(p, d_x_inout, init, nullptr, max_iter, xtol, lambda0, d_status, d_cost, st));
  return block_counts(p->pts, counts, iters_max, st);
}

extern "C" int ba_refine_points(ba_problem *p, double *x_inout, int init, int max_iter, double xtol, double lambda0, uint8_t *status,
                                double *cost, int64_t *counts, int *iters_max) {
  BA_CHECK(refine_check("ba_refine_points", p, x_inout, init, &max_iter, &xtol, &lambda0));
  // the points only: the camera part of the caller's x is never written
  return block_host_entry(p, p->pts, x_inout, p->npnts, 3, 0, status, cost, counts, iters_max,
                          [&](double *dx, uint8_t *d_status, double *d_cost, hipStream_t st) {
                            return refine_launch(p, dx, init, nullptr, max_iter, xtol, lambda0, d_status, d_cost, st);
                          });
}

// ---- ba_ransac_points: a consensus stage in front of ba_refine_points(init = 1) ------------------------------------
// the consensus results of the last call -> the caller's arrays (each may be null), on st
static int ransac_results(ba_problem *p, uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp, hipMemcpyKind kind, hipStream_t st) {
  const PointWork &w = p->pts;
  if (p->npnts == 0) return BA_OK;
  if (inlier && p->nobs > 0) BA_HIP_CHECK(hipMemcpyAsync(inlier, w.rs_inlier, (size_t)p->nobs, kind, st));
  if (n_inliers) BA_HIP_CHECK(hipMemcpyAsync(n_inliers, w.rs_n, (size_t)p->npnts * sizeof(int32_t), kind, st));
  if (best_hyp) BA_HIP_CHECK(hipMemcpyAsync(best_hyp, w.rs_best, (size_t)p->npnts * sizeof(int32_t), kind, st));
  return BA_OK;
}

// the options (a sample of exactly two observations, a set of at least two), then the refusals of ba_refine_points
static int ransac_check(const char *who, ba_problem *p, const double *x, const ba_ransac_opts *opts, ba_ransac_opts *o, int *max_iter,
                        double *xtol, double *lambda0) {
  BA_CHECK(ransac_opts_check(who, opts, o, 2, 2, 2));
  return refine_check(who, p, x, 1, max_iter, xtol, lambda0);
}

extern "C" int ba_ransac_points_dev(ba_problem *p, double *d_x_inout, const ba_ransac_opts *opts, int max_iter, double xtol,
                                    double lambda0, uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max,
                                    uint8_t *d_inlier, int32_t *d_n_inliers, int32_t *d_best_hyp, void *stream) {
  ba_ransac_opts o;
  BA_CHECK(ransac_check("ba_ransac_points_dev", p, d_x_inout, opts, &o, &max_iter, &xtol, &lambda0));
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)p->stream;
  BA_CHECK(refine_launch(p, d_x_inout, 1, &o, max_iter, xtol, lambda0, d_status, d_cost, st));
  BA_CHECK(ransac_results(p, d_inlier, d_n_inliers, d_best_hyp, hipMemcpyDeviceToDevice, st));
  return block_counts(p->pts, counts, iters_max, st);
}

extern "C" int ba_ransac_points(ba_problem *p, double *x_inout, const ba_ransac_opts *opts, int max_iter, double xtol, double lambda0,
                                uint8_t *status, double *cost, int64_t *counts, int *iters_max, uint8_t *inlier, int32_t *n_inliers,
                                int32_t *best_hyp) {
  ba_ransac_opts o;
  BA_CHECK(ransac_check("ba_ransac_points", p, x_inout, opts, &o, &max_iter, &xtol, &lambda0));
  return block_host_entry(p, p->pts, x_inout, p->npnts, 3, 0, status, cost, counts, iters_max,
                          [&](double *dx, uint8_t *d_status, double *d_cost, hipStream_t st) {
                            BA_CHECK(refine_launch(p, dx, 1, &o, max_iter, xtol, lambda0, d_status, d_cost, st));
                            return ransac_results(p, inlier, n_inliers, best_hyp, hipMemcpyDeviceToHost, st);
                          });
}
