// Cameras with the points held (ba_refine_cameras): a per-camera Marquardt iteration on the handle's objective
// restricted to one camera.  gfx950 only.
//
// With every point entry of x held, camera c is an independent problem in at most 9 unknowns:
//   f_c(C) = sum_{o in obs(c)} 1/2 c^2 rho(r^_o' r^_o / c^2) + 1/2 (C - mu)' Lambda_cam (C - mu)
//            + 1/2 (c(C) - mu')' Lambda_ctr (c(C) - mu')
// (rho, c: ba_lm_set_loss; r^ = L'r: ba_lm_set_obs_info; the second term for a camera with a camera prior, the third for one with
// a centre prior, c(C) = -R(r)'t).  ONE launch runs the whole refinement: the iteration loop is inside k_refine_cameras.  The
// residual and the camera columns of the Jacobian are the model's own device functions (ba_model_dev.h): jac_block is inlined
// and only its columns 3..11 are used; the centre and its Jacobian are centre_of (ba_prior_dev.h).
//
// One 256-lane workgroup per camera, whatever its degree (the argument: DESIGN §5k).  The lanes stride over the camera's list
// cam_ptr[c] .. cam_ptr[c + 1] of cam_obs, gather the held points from x and keep the 55 sums of an evaluation (f, g, the packed
// lower H) in registers; the sums go through an xor butterfly inside each wave and through LDS across the four waves, always as
// ((w0 + w1) + w2) + w3, so a camera's result depends on nothing but its own data and the order of its list.  Thread 0 then
// runs the 9 x 9 algebra (priors, masking, damping, Cholesky, the two triangular solves, the scaled norms, the accept test) on
// LDS-resident arrays and leaves the next trial camera and its cam_pre row in LDS for all lanes: the camera's trigonometry is
// evaluated once per trial.  No floating-point atomics; the eight counters of a call are integers, added once per workgroup.
//
// ba_resect_cameras launches k_resect_cameras before it: the start pose of every camera whose pose is free, in
// closed form from its 2D-3D correspondences (further down).  ba_ransac_cameras puts the consensus kernels of
// ba_ransac_kernels.hip in front of both and hands them its inlier set as information (ransac_consensus, on the host side).
// The _focal entries are the same launches with CamArgs.focal set: a camera whose f is free gets it from the
// resection's eigenvector as well, every other camera is handled as before.
//
// What this file has in common with ba_point_kernels.hip is written once: the device pieces in ba_refine_dev.h, the host side
// (argument check, prior lookups, counter read-back, the body of the host-pointer entries; BlockWork) in ba_internal.h / ba_api.hip.
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

#include "ba_model_dev.h"  // CPAD, cam_pre, project_pre, jac_block
#include "ba_prior_dev.h"  // centre_of
#include "ba_refine_dev.h"  // wave_all_sum, p1_z, the pieces of the linear resection

constexpr int CM_BLK = 256, CM_WAVES = CM_BLK / 64;
constexpr int CM_SUMS = 55;                     // [f | g (9) | H (45, packed lower row-major)]
constexpr int CM_G = 1, CM_H = 10;              // where g and H start
constexpr unsigned CM_ALL = 0x1FFu, CM_INTRINSICS = 0x1C0u;  // (the pose components: POSE_MASK)
enum { RS_DONE = 0, RS_SKIPPED = 1, RS_DEGENERATE = 2 };  // the byte per camera k_resect_cameras leaves for k_refine_cameras

struct CamArgs {
  const int *cam_ptr, *cam_obs, *pnt0;
  const double *pt2d, *info;          // info: l00 l10 l11 per observation, or null
  const uint16_t *mask;               // effective mask of held components per camera, or null
  const int *cam_pri_of, *ctr_pri_of; // camera -> its camera / centre prior, -1: none; or null
  const double *cam_mu, *cam_info, *ctr_mu, *ctr_info;
  const double *x;                    // the whole vector (the points are read from it)
  double *xc;                         // its camera part
  uint8_t *status;                    // or null
  uint8_t *resect;                    // what k_resect_cameras did per camera (RS_*), or null: no resection ran
  int focal;                          // the resection estimates f for every camera whose f is free (ba_resect_cameras_focal)
  double *cost;                       // or null
  unsigned long long *counts;
  int max_iter, kind;
  double xtol, lambda0, c2;
};

struct CamShared {
  double red[CM_WAVES][CM_SUMS + 1];  // the waves' sums of an evaluation
  int redb[CM_WAVES], redu[CM_WAVES]; // ... an observation behind the camera, an observation with Lambda != 0
  double C[9], Cn[9], P[12];          // the camera, the trial camera and the trial's cam_pre row
  double S[CM_SUMS], Sn[CM_SUMS];     // f, g, H at C and at the trial (priors included)
  double A[45], y[9], d[9], D[9];     // damped matrix / its Cholesky factor, the solves, D_j = sqrt(H_jj) of the step's H
  double e[9], w[9], Hc[18], M[18];   // prior terms
  int stop;
};

// cam_pre row of the trial camera sh.Cn -> sh.P (one lane)
__device__ __forceinline__ void trial_row(CamShared &sh) {
  double C9[9], P[12];
#pragma unroll
  for (int i = 0; i < 9; i++) C9[i] = sh.Cn[i];
  cam_pre<double>(C9, P);
#pragma unroll
  for (int i = 0; i < 12; i++) sh.P[i] = P[i];
}

// The observation sums of camera list [k0, k1) at the trial camera (row sh.P), all lanes: wave w's sums -> sh.red[w], whether
// one of its observations with Lambda != 0 has P1.z >= 0 -> sh.redb[w], whether it has such an observation at all -> sh.redu[w]
__device__ __forceinline__ void observation_sums(const CamArgs &a, CamShared &sh, int k0, int k1, int t) {
  double P[12], acc[CM_SUMS];
#pragma unroll
  for (int i = 0; i < 12; i++) P[i] = sh.P[i];
#pragma unroll
  for (int i = 0; i < CM_SUMS; i++) acc[i] = 0.0;
  int bh = 0, used = 0;
  for (int k = k0 + t; k < k1; k += CM_BLK) {
    const int o = a.cam_obs[k];
    double l00 = 1.0, l10 = 0.0, l11 = 1.0;
    if (a.info) l00 = a.info[3 * (int64_t)o], l10 = a.info[3 * (int64_t)o + 1], l11 = a.info[3 * (int64_t)o + 2];
    if (l00 == 0.0 && l10 == 0.0 && l11 == 0.0) continue;  // Lambda = 0: the observation is dropped
    used = 1;
    const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
    const double X[3] = {xp[0], xp[1], xp[2]};
    const double2 m = reinterpret_cast<const double2 *>(a.pt2d)[o];
    double out[2], J[24];
    project_pre<double>(X, P, out);
    jac_block<double>(X, P, J);  // (columns 3..11 of both rows are used: R, the point columns, is dead code)
    double z1;
    p1_z(P, X, z1);
    if (z1 >= 0.0) bh = 1;
    const double ex = out[0] - m.x, ey = out[1] - m.y;
    const double rx = l00 * ex + l10 * ey, ry = l11 * ey;
    double w;
    acc[0] += robust_rho(a.kind, rx * rx + ry * ry, a.c2, &w);
    double j0[9], j1[9], wj0[9], wj1[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      j0[i] = l00 * J[3 + i] + l10 * J[15 + i];
      j1[i] = l11 * J[15 + i];
      wj0[i] = w * j0[i];
      wj1[i] = w * j1[i];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
      acc[CM_G + i] += wj0[i] * rx + wj1[i] * ry;
#pragma unroll
      for (int j = 0; j <= i; j++) acc[CM_H + i * (i + 1) / 2 + j] += wj0[i] * j0[j] + wj1[i] * j1[j];
    }
  }
#pragma unroll
  for (int i = 0; i < CM_SUMS; i++) acc[i] = wave_all_sum(acc[i]);
  bh = __any(bh) ? 1 : 0;
  used = __any(used) ? 1 : 0;
  if ((t & 63) == 0) {
    const int wv = t >> 6;
#pragma unroll
    for (int i = 0; i < CM_SUMS; i++) sh.red[wv][i] = acc[i];
    sh.redb[wv] = bh;
    sh.redu[wv] = used;
  }
}

// f, g, H at the trial camera -> sh.Sn: the waves' sums in wave order, then the camera prior qc and the centre prior qt (-1: none)
// (one lane)
__device__ __forceinline__ void trial_totals(const CamArgs &a, CamShared &sh, int qc, int qt) {
  for (int i = 0; i < CM_SUMS; i++) sh.Sn[i] = ((sh.red[0][i] + sh.red[1][i]) + sh.red[2][i]) + sh.red[3][i];
  sh.Sn[0] *= 0.5;
  if (qc >= 0) {
    const double *mu = a.cam_mu + 9 * (int64_t)qc, *L = a.cam_info + 45 * (int64_t)qc;
    for (int i = 0; i < 9; i++) {
      sh.e[i] = sh.Cn[i] - mu[i];
      sh.w[i] = 0.0;
    }
    int tt = 0;
    for (int i = 0; i < 9; i++)
      for (int j = 0; j <= i; j++, tt++) {
        const double v = L[tt];
        sh.w[i] += v * sh.e[j];
        if (j < i) sh.w[j] += v * sh.e[i];
        sh.Sn[CM_H + tt] += v;
      }
    double q = 0.0;
    for (int i = 0; i < 9; i++) {
      q += sh.e[i] * sh.w[i];
      sh.Sn[CM_G + i] += sh.w[i];
    }
    sh.Sn[0] += 0.5 * q;
  }
  if (qt >= 0) {
    const double *mu = a.ctr_mu + 3 * (int64_t)qt, *L = a.ctr_info + 6 * (int64_t)qt;
    double C6[6], ctr[3], H[18];
#pragma unroll
    for (int i = 0; i < 6; i++) C6[i] = sh.Cn[i];
    centre_of<true>(C6, ctr, H);
#pragma unroll
    for (int i = 0; i < 18; i++) sh.Hc[i] = H[i];
    const double e0 = ctr[0] - mu[0], e1 = ctr[1] - mu[1], e2 = ctr[2] - mu[2];
    const double w0 = L[0] * e0 + L[1] * e1 + L[3] * e2, w1 = L[1] * e0 + L[2] * e1 + L[4] * e2, w2 = L[3] * e0 + L[4] * e1 + L[5] * e2;
    sh.Sn[0] += 0.5 * (e0 * w0 + e1 * w1 + e2 * w2);
    for (int j = 0; j < 6; j++) {  // M = Lambda H
      const double h0 = sh.Hc[j], h1 = sh.Hc[6 + j], h2 = sh.Hc[12 + j];
      sh.M[j] = L[0] * h0 + L[1] * h1 + L[3] * h2;
      sh.M[6 + j] = L[1] * h0 + L[2] * h1 + L[4] * h2;
      sh.M[12 + j] = L[3] * h0 + L[4] * h1 + L[5] * h2;
    }
    int tt = 0;  // (the leading 6 x 6 of the packed lower H is its first 21 entries)
    for (int i = 0; i < 6; i++) {
      for (int j = 0; j <= i; j++, tt++)
        sh.Sn[CM_H + tt] += (sh.Hc[i] * sh.M[j] + sh.Hc[6 + i] * sh.M[6 + j]) + sh.Hc[12 + i] * sh.M[12 + j];
      sh.Sn[CM_G + i] += (sh.Hc[i] * w0 + sh.Hc[6 + i] * w1) + sh.Hc[12 + i] * w2;
    }
  }
}

// (H + lam diag H) delta = -g at sh.S with the rows and columns of the held components fm replaced by the identity, by a 9 x 9
// Cholesky: delta -> sh.d, D_j = sqrt(H_jj) (0: held) -> sh.D.  False: a pivot that is not positive or not finite, or a
// delta that is not finite.  (one lane)
__device__ __forceinline__ bool damped_step(CamShared &sh, unsigned fm, double lam) {
  int tt = 0;
  for (int i = 0; i < 9; i++)
    for (int j = 0; j <= i; j++, tt++) {
      const bool held = (((fm >> i) | (fm >> j)) & 1u) != 0;
      double v = held ? (i == j ? 1.0 : 0.0) : sh.S[CM_H + tt];
      if (i == j) v += lam * v;
      sh.A[tt] = v;
    }
  for (int i = 0; i < 9; i++) {
    const int ri = i * (i + 1) / 2;
    for (int j = 0; j <= i; j++) {
      const int rj = j * (j + 1) / 2;
      double s = sh.A[ri + j];
      for (int k = 0; k < j; k++) s -= sh.A[ri + k] * sh.A[rj + k];
      if (i == j) {
        if (!(s > 0.0) || !isfinite(s)) return false;
        sh.A[ri + i] = sqrt(s);
      } else {
        sh.A[ri + j] = s / sh.A[rj + j];
      }
    }
  }
  for (int i = 0; i < 9; i++) {  // L y = -g
    const int ri = i * (i + 1) / 2;
    double s = ((fm >> i) & 1u) ? 0.0 : -sh.S[CM_G + i];
    for (int k = 0; k < i; k++) s -= sh.A[ri + k] * sh.y[k];
    sh.y[i] = s / sh.A[ri + i];
  }
  bool finite = true;
  for (int i = 8; i >= 0; i--) {  // L' delta = y
    double s = sh.y[i];
    for (int k = i + 1; k < 9; k++) s -= sh.A[k * (k + 1) / 2 + i] * sh.d[k];
    sh.d[i] = s / sh.A[i * (i + 1) / 2 + i];
    finite = finite && isfinite(sh.d[i]);
  }
  for (int i = 0; i < 9; i++) sh.D[i] = ((fm >> i) & 1u) ? 0.0 : sqrt(sh.S[CM_H + i * (i + 1) / 2 + i]);
  return finite;
}

// One camera per workgroup.  The control flow is uniform over the workgroup: thread 0 decides, sh.stop tells.
__global__ __launch_bounds__(CM_BLK) void k_refine_cameras(CamArgs a) {
  __shared__ CamShared sh;
  const int t = threadIdx.x;
  const int c = (int)blockIdx.x;
  const int k0 = a.cam_ptr[c], k1 = a.cam_ptr[c + 1];
  double *xc = a.xc + 9 * (int64_t)c;
  const unsigned fm = a.mask ? (unsigned)a.mask[c] : 0u;
  const int qc = a.cam_pri_of ? a.cam_pri_of[c] : -1, qt = a.ctr_pri_of ? a.ctr_pri_of[c] : -1;
  // (thread 0's state)
  int status = BA_PT_DEGENERATE, trials = 0, behind = 0;
  bool write = false;
  double fb = 0.0, lam = a.lambda0;
  if (a.resect && a.resect[c] == RS_DEGENERATE) {  // no pose was found: DEGENERATE, the camera untouched, cost entries 0, no flag
    if (t == 0) {
      if (a.status) a.status[c] = (uint8_t)BA_PT_DEGENERATE;
      if (a.cost) a.cost[2 * (int64_t)c] = 0.0, a.cost[2 * (int64_t)c + 1] = 0.0;
      atomicAdd(a.counts + BA_PT_DEGENERATE, 1ull);
    }
    return;
  }
  if (t == 0) {
    for (int i = 0; i < 9; i++) sh.C[i] = sh.Cn[i] = xc[i];
    trial_row(sh);
    sh.stop = 0;
  }
  __syncthreads();
  for (int it = -1;; it++) {  // it = -1: the evaluation at the start; it >= 0: the evaluation of a trial
    observation_sums(a, sh, k0, k1, t);
    __syncthreads();
    if (t == 0) {
      trial_totals(a, sh, qc, qt);
      const int bn = sh.redb[0] | sh.redb[1] | sh.redb[2] | sh.redb[3];
      const double fn = sh.Sn[0];
      bool stop = false;
      if (it < 0) {
        const int used = sh.redu[0] | sh.redu[1] | sh.redu[2] | sh.redu[3];
        for (int i = 0; i < CM_SUMS; i++) sh.S[i] = sh.Sn[i];
        fb = fn;
        behind = bn;
        if (fm == CM_ALL) {
          status = BA_PT_FIXED;
          stop = true;
        } else if (!used && qc < 0 && qt < 0) {  // nothing constrains the camera: DEGENERATE, cost entries 0, no flag
          sh.S[0] = fb = 0.0;
          behind = 0;
          stop = true;
        } else if (!isfinite(fn)) {
          status = BA_PT_NONFINITE;
          behind = 0;
          stop = true;
        } else {
          status = BA_PT_MAX_ITER;
          stop = a.max_iter == 0;
        }
      } else if (fn <= sh.S[0]) {  // accepted (false for a NaN)
        for (int i = 0; i < 9; i++) sh.C[i] = sh.Cn[i];
        for (int i = 0; i < CM_SUMS; i++) sh.S[i] = sh.Sn[i];
        behind = bn;
        write = true;
        lam = fmax(lam / 10.0, 1e-12);
        double nd = 0.0, nx = 0.0;
        for (int i = 0; i < 9; i++) {
          const double u = sh.D[i] * sh.d[i], v = sh.D[i] * sh.C[i];
          nd += u * u;
          nx += v * v;
        }
        if (sqrt(nd) <= a.xtol * (sqrt(nx) + a.xtol)) {
          status = BA_PT_CONVERGED;
          stop = true;
        } else {
          stop = trials >= a.max_iter;
        }
      } else {
        lam *= 10.0;
        if (lam > 1e12) {
          status = BA_PT_STALLED;
          stop = true;
        } else {
          stop = trials >= a.max_iter;
        }
      }
      while (!stop) {  // the next trial; a step that cannot be solved is a rejected trial without an evaluation
        trials++;
        if (damped_step(sh, fm, lam)) {
          for (int i = 0; i < 9; i++) sh.Cn[i] = ((fm >> i) & 1u) ? sh.C[i] : sh.C[i] + sh.d[i];
          trial_row(sh);
          break;
        }
        lam *= 10.0;
        if (lam > 1e12) {
          status = BA_PT_STALLED;
          stop = true;
        } else {
          stop = trials >= a.max_iter;
        }
      }
      sh.stop = stop ? 1 : 0;
    }
    __syncthreads();
    if (sh.stop) break;
  }
  if (t == 0) {
    const int st = status | (behind ? BA_PT_BEHIND : 0);
    if (write)
      for (int i = 0; i < 9; i++) xc[i] = sh.C[i];
    if (a.status) a.status[c] = (uint8_t)st;
    if (a.cost) a.cost[2 * (int64_t)c] = fb, a.cost[2 * (int64_t)c + 1] = sh.S[0];
    atomicAdd(a.counts + status, 1ull);
    if (behind) atomicAdd(a.counts + BA_PT_STATES, 1ull);
    atomicMax(a.counts + BA_PT_STATES + 1, (unsigned long long)trials);
  }
}

// ---- linear resection (ba_resect_cameras): the start pose of a camera from its 2D-3D correspondences ------------
// The steps are those of ba_refine_dev.h; here the lanes of a workgroup stride over the camera's list, 40 sums per lane, reduced
// as observation_sums reduces its 55.
struct RsShared {
  double red[CM_WAVES][RS_SUMS];
  int first[CM_WAVES], front;
  ResectScratch rs;
};

// The sums acc of all lanes -> every lane: xor butterfly per wave, LDS across the waves, ((w0 + w1) + w2) + w3
template <int N>
__device__ __forceinline__ void block_sums(double (&acc)[N], RsShared &sh, int t) {
#pragma unroll
  for (int i = 0; i < N; i++) acc[i] = wave_all_sum(acc[i]);
  __syncthreads();  // (the readers of the sums before these are done)
  if ((t & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) sh.red[t >> 6][i] = acc[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; i++) acc[i] = ((sh.red[0][i] + sh.red[1][i]) + sh.red[2][i]) + sh.red[3][i];
}

// One camera per workgroup: the pose (r, t) of xc from the camera's observations with Lambda != 0, its intrinsics and the held
// points; the pose of x is not read.  a.resect[c] <- RS_DONE (pose written), RS_SKIPPED (a pose component is held: nothing is
// done) or RS_DEGENERATE (nothing written).  In focal mode (a.focal and the camera's f free) the intrinsics are not
// read either: the measurements are scaled by the image scale, f comes out of the eigenvector and is written with the pose,
// a free k1 / k2 as 0.  The control flow is uniform over the workgroup.
__global__ __launch_bounds__(CM_BLK) void k_resect_cameras(CamArgs a) {
  __shared__ RsShared sh;
  const int t = threadIdx.x;
  const int c = (int)blockIdx.x;
  const int k0 = a.cam_ptr[c], k1 = a.cam_ptr[c + 1];
  double *xc = a.xc + 9 * (int64_t)c;
  const unsigned fm = a.mask ? (unsigned)a.mask[c] : 0u;
  if (fm & POSE_MASK) {
    if (t == 0) a.resect[c] = RS_SKIPPED;
    return;
  }
  const bool focal = focal_mode(a.focal, fm);
  const double ck1 = xc[6], ck2 = xc[7];
  double cf = xc[8];  // (focal mode: not used; the image scale takes its place)
  // the provisional origin: the point of the first observation of the list with Lambda != 0
  int first = k1;
  for (int k = k0 + t; k < k1; k += CM_BLK)
    if (obs_used(a.info, a.cam_obs[k])) {
      first = k;
      break;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
  if ((t & 63) == 0) sh.first[t >> 6] = first;
  if (t == 0) sh.front = 0;
  __syncthreads();
  first = min(min(sh.first[0], sh.first[1]), min(sh.first[2], sh.first[3]));
  if (first >= k1 || (!focal && (!isfinite(cf) || cf == 0.0))) {
    if (t == 0) a.resect[c] = RS_DEGENERATE;
    return;
  }
  double org[3];
  {
    const double *xp = a.x + 3 * (int64_t)a.pnt0[a.cam_obs[first]];
    org[0] = xp[0], org[1] = xp[1], org[2] = xp[2];
  }
  // the number of used observations, their mean and their RMS distance from it; focal mode: sum |m|^2 as well, reduced on its
  // own so that the calibrated path keeps its five sums
  double mo[5] = {0, 0, 0, 0, 0}, sm2[1] = {0};
  for (int k = k0 + t; k < k1; k += CM_BLK) {
    const int o = a.cam_obs[k];
    if (!obs_used(a.info, o)) continue;
    const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
    const double d0 = xp[0] - org[0], d1 = xp[1] - org[1], d2 = xp[2] - org[2];
    mo[0] += 1.0;
    mo[1] += d0, mo[2] += d1, mo[3] += d2;
    mo[4] += (d0 * d0 + d1 * d1) + d2 * d2;
    if (focal) {
      const double2 m = reinterpret_cast<const double2 *>(a.pt2d)[o];
      sm2[0] += m.x * m.x + m.y * m.y;
    }
  }
  block_sums<5>(mo, sh, t);
  if (focal) block_sums<1>(sm2, sh, t);
  const double n = mo[0];
  double dm[3], sc;
  if (n < (double)RS_MIN_OBS || !hartley_stats(n, mo + 1, mo[4], dm, sc) || (focal && !image_scale(n, sm2[0], cf))) {
    if (t == 0) a.resect[c] = RS_DEGENERATE;
    return;
  }
  // the moments
  double acc[RS_SUMS];
#pragma unroll
  for (int i = 0; i < RS_SUMS; i++) acc[i] = 0.0;
  for (int k = k0 + t; k < k1; k += CM_BLK) {
    const int o = a.cam_obs[k];
    if (!obs_used(a.info, o)) continue;
    const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
    const double X[3] = {xp[0], xp[1], xp[2]};
    const double2 m = reinterpret_cast<const double2 *>(a.pt2d)[o];
    double h[4], qx, qy, term[RS_SUMS];
    normalised_point(X, org, dm, sc, h);
    if (focal) qx = m.x / cf, qy = m.y / cf;
    else undistort(m.x / cf, m.y / cf, ck1, ck2, qx, qy);
    moment_terms(h, qx, qy, term);
#pragma unroll
    for (int i = 0; i < RS_SUMS; i++) acc[i] += term[i];
  }
  block_sums<RS_SUMS>(acc, sh, t);
  if (t == 0) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < RS_SUMS; i++) {
      ok = ok && isfinite(acc[i]);
      sh.rs.S[i] = acc[i];
    }
    sh.rs.ok = ok ? 1 : 0;
  }
  __syncthreads();
  if (!sh.rs.ok) {
    if (t == 0) a.resect[c] = RS_DEGENERATE;
    return;
  }
  for (int e = t; e < 144; e += CM_BLK) sh.rs.M[e] = normal_matrix_entry(sh.rs.S, e);
  jacobi12<__syncthreads>(sh.rs.M, sh.rs.V, t, CM_BLK);
  int i1;
  if (!smallest_eigenpair(sh.rs.M, i1)) {  // (every lane reads the same diagonal)
    if (t == 0) a.resect[c] = RS_DEGENERATE;
    return;
  }
  {  // the used points in front of the camera under the eigenvector's sign
    int front = 0;
    for (int k = k0 + t; k < k1; k += CM_BLK) {
      const int o = a.cam_obs[k];
      if (!obs_used(a.info, o)) continue;
      const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
      const double X[3] = {xp[0], xp[1], xp[2]};
      double h[4];
      normalised_point(X, org, dm, sc, h);
      if (front_z(sh.rs.V, i1, h) < 0.0) front++;
    }
    if (front) atomicAdd(&sh.front, front);
  }
  __syncthreads();
  if (t == 0) {
    const double sgn = 2.0 * (double)sh.front >= n ? 1.0 : -1.0;
    const bool ok = (!focal || focal_from_eigenvector(sh.rs, i1, cf)) && pose_from_eigenvector(sh.rs, i1, sgn, sc, org, dm);
    if (ok) {
      xc[0] = sh.rs.r[0], xc[1] = sh.rs.r[1], xc[2] = sh.rs.r[2];
      xc[3] = sh.rs.tr[0], xc[4] = sh.rs.tr[1], xc[5] = sh.rs.tr[2];
      if (focal) {  // f^ = a phi; a free k1 / k2 starts at 0, a held one keeps its bits (the linear stage ignores it)
        if (!(fm & K1_HELD)) xc[6] = 0.0;
        if (!(fm & K2_HELD)) xc[7] = 0.0;
        xc[8] = sh.rs.f;
      }
    }
    a.resect[c] = ok ? RS_DONE : RS_DEGENERATE;
  }
}

}  // namespace

// where a call's cameras start: from x (ba_refine_cameras), from the linear resection with the intrinsics of x
// (ba_resect_cameras, ba_ransac_cameras), or from the resection that estimates f as well (the _focal entries)
enum CamStart { START_X = 0, START_RESECT, START_FOCAL };

// the per-camera lookups of the priors (once per ba_lm_set_priors) and the effective mask (once per ba_lm_set_fixed /
// ba_lm_set_shared_intrinsics)
static int camera_tables(ba_problem *p) {
  CameraWork &w = p->cams;
  if (!w.counts) BA_CHECK(w.counts.alloc(BLOCK_COUNTERS));
  if (w.pri_version != p->pri_version) {
    BA_CHECK(block_prior_lookup(p->pri[PRI_CAM], p->ncams, w.cam_pri_of));
    BA_CHECK(block_prior_lookup(p->pri[PRI_CTR], p->ncams, w.ctr_pri_of));
    w.pri_version = p->pri_version;
  }
  if (w.fix_version != p->fix_version || w.grp_version != p->grp_version) {
    w.mask_on = p->fix_ncam > 0 || p->grp_on();
    if (w.mask_on) {
      std::vector<uint16_t> m((size_t)p->ncams, 0);
      for (int64_t c = 0; c < p->ncams; c++) {
        if (p->fix_ncam > 0) m[(size_t)c] = p->h_fix_cam[(size_t)c];
        if (p->grp_on() && p->h_grp[(size_t)c] > 0) m[(size_t)c] |= (uint16_t)CM_INTRINSICS;
      }
      BA_CHECK(upload(w.mask, m));
    }
    w.fix_version = p->fix_version;
    w.grp_version = p->grp_version;
  }
  return BA_OK;
}

static int camera_check(const char *who, ba_problem *p, const double *x, int *max_iter, double *xtol, double *lambda0) {
  return block_check(who, p, x, 100, max_iter, xtol, lambda0, [&] {
    if (!p->comm.active()) return BA_OK;
    ba_set_error("%s: not supported on a handle with a communicator (a camera's observations are spread over the shards)", who);
    return BA_ERR_ARG;
  });
}

// the arguments of k_resect_cameras / k_refine_cameras on d_x from the handle's terms (after terms_upload and camera_tables)
static CamArgs camera_args(ba_problem *p, double *d_x, CamStart start, int max_iter, double xtol, double lambda0, uint8_t *d_status,
                           double *d_cost) {
  CameraWork &w = p->cams;
  const PriorSet &cm = p->pri[PRI_CAM], &ct = p->pri[PRI_CTR];
  CamArgs a;
  a.cam_ptr = p->cam_ptr, a.cam_obs = p->cam_obs, a.pnt0 = p->pnt0;
  a.pt2d = p->pt2d, a.info = p->info_on() ? (const double *)p->d_info : nullptr;
  a.mask = w.mask_on ? (const uint16_t *)w.mask : nullptr;
  a.cam_pri_of = cm.n > 0 ? (const int *)w.cam_pri_of : nullptr, a.ctr_pri_of = ct.n > 0 ? (const int *)w.ctr_pri_of : nullptr;
  a.cam_mu = cm.n > 0 ? (const double *)cm.mu : nullptr, a.cam_info = cm.n > 0 ? (const double *)cm.info : nullptr;
  a.ctr_mu = ct.n > 0 ? (const double *)ct.mu : nullptr, a.ctr_info = ct.n > 0 ? (const double *)ct.info : nullptr;
  a.x = d_x, a.xc = d_x + 3 * p->npnts, a.status = d_status, a.cost = d_cost, a.counts = w.counts;
  a.resect = start != START_X ? (uint8_t *)w.resect : nullptr;
  a.focal = start == START_FOCAL ? 1 : 0;
  a.max_iter = max_iter, a.kind = p->loss;
  a.xtol = xtol, a.lambda0 = lambda0, a.c2 = p->loss_scale * p->loss_scale;
  return a;
}

static int launch_resect(ba_problem *p, const CamArgs &a, hipStream_t st) {
  ProfScope ps(p, PC_RESECT_CAMERAS, st);
  return BA_LAUNCH(k_resect_cameras, (unsigned)p->ncams, CM_BLK, 0, st, a);
}

static int launch_refine(ba_problem *p, const CamArgs &a, hipStream_t st) {
  ProfScope ps(p, PC_REFINE_CAMERAS, st);
  return BA_LAUNCH(k_refine_cameras, (unsigned)p->ncams, CM_BLK, 0, st, a);
}

// the arguments of the consensus kernels (ba_ransac_kernels.hip) from those of the camera kernels
static RansacArgs ransac_args(ba_problem *p, const CamArgs &a, const ba_ransac_opts &o) {
  CameraWork &w = p->cams;
  RansacArgs r;
  r.cam_ptr = a.cam_ptr, r.cam_obs = a.cam_obs, r.pnt0 = a.pnt0, r.pt2d = a.pt2d, r.info = a.info, r.mask = a.mask;
  r.x = a.x, r.xc = a.xc, r.hyp_pose = w.hyp_pose, r.hyp_count = w.hyp_count;
  r.inlier = w.rs_inlier, r.stopped = w.rs_stopped, r.n_inliers = w.rs_n, r.best_hyp = w.rs_best;
  r.hypotheses = o.hypotheses, r.sample = o.sample, r.min_inliers = o.min_inliers;
  r.seed_mix = ransac_seed_mix(o.seed), r.tau2 = o.threshold * o.threshold;
  r.focal = a.focal;
  return r;
}

// The consensus stage of ba_ransac_cameras: hypotheses -> select -> refits x (mask -> resect into the scratch
// cameras -> rescore) -> mask; gen: what solves a hypothesis, the one thing ba_ransac_cameras_p3p changes.  The set
// reaches k_resect_cameras and k_refine_cameras as information: w.rs_info, the masked copy of the factors (1 0 1 when the caller
// set none: the values the kernels use without an array).
static int ransac_consensus(ba_problem *p, const CamArgs &a, const ba_ransac_opts &o, RansacGen gen, hipStream_t st) {
  CameraWork &w = p->cams;
  if (!w.rs_inlier) {
    BA_CHECK(w.rs_inlier.alloc(p->nobs));
    BA_CHECK(w.rs_info.alloc(3 * p->nobs));
    BA_CHECK(w.rs_cams.alloc(9 * p->ncams));
    BA_CHECK(w.rs_n.alloc(p->ncams));
    BA_CHECK(w.rs_best.alloc(p->ncams));
    BA_CHECK(w.rs_stopped.alloc(p->ncams));
  }
  if (w.hyp_cap < o.hypotheses) {
    w.hyp_cap = 0;
    BA_CHECK(w.hyp_pose.alloc(RANSAC_HYP_DOUBLES * p->ncams * o.hypotheses));
    BA_CHECK(w.hyp_count.alloc(p->ncams * o.hypotheses));
    w.hyp_cap = o.hypotheses;
  }
  const RansacArgs r = ransac_args(p, a, o);
  {
    ProfScope ps(p, PC_RANSAC_CAMERAS, st);
    BA_CHECK(launch_ransac_hypotheses(r, p->ncams, gen, st));
    BA_CHECK(launch_ransac_select(r, p->ncams, st));
  }
  // the refits on the set: their poses (focal mode: and f^) live in a scratch copy of the cameras (the intrinsics are read from it)
  CamArgs fit = a;
  fit.info = w.rs_info, fit.xc = w.rs_cams;
  if (o.refits > 0)
    BA_HIP_CHECK(hipMemcpyAsync(w.rs_cams, a.xc, (size_t)(9 * p->ncams) * sizeof(double), hipMemcpyDeviceToDevice, st));
  for (int it = 0; it < o.refits; it++) {
    {
      ProfScope ps(p, PC_RANSAC_CAMERAS, st);
      BA_CHECK(launch_ransac_mask_info(r, p->nobs, w.rs_info, st));
    }
    BA_CHECK(launch_resect(p, fit, st));
    ProfScope ps(p, PC_RANSAC_CAMERAS, st);
    BA_CHECK(launch_ransac_rescore(r, p->ncams, w.rs_cams, w.resect, st));
  }
  ProfScope ps(p, PC_RANSAC_CAMERAS, st);
  return launch_ransac_mask_info(r, p->nobs, w.rs_info, st);
}

// (ransac: the consensus stage, which leaves its set as information, then) (start != START_X: k_resect_cameras, the start poses
// -- START_FOCAL: and focal lengths -- written into d_x, then) k_refine_cameras, on st without a host synchronisation; the
// counters stay on the device (p->cams.counts)
static int camera_launch(ba_problem *p, double *d_x, CamStart start, const ba_ransac_opts *ransac, RansacGen gen, int max_iter,
                         double xtol, double lambda0, uint8_t *d_status, double *d_cost, hipStream_t st) {
  BA_CHECK(terms_upload(p));
  BA_CHECK(camera_tables(p));
  CameraWork &w = p->cams;
  BA_HIP_CHECK(hipMemsetAsync(w.counts, 0, BLOCK_COUNTERS * sizeof(unsigned long long), st));
  if (p->ncams == 0) return BA_OK;
  if (start != START_X && !w.resect) BA_CHECK(w.resect.alloc(p->ncams));
  CamArgs a = camera_args(p, d_x, start, max_iter, xtol, lambda0, d_status, d_cost);
  if (ransac) {
    BA_CHECK(ransac_consensus(p, a, *ransac, gen, st));
    a.info = w.rs_info;
  }
  if (start != START_X) BA_CHECK(launch_resect(p, a, st));
  return launch_refine(p, a, st);
}

static int refine_cameras_dev(const char *who, ba_problem *p, double *d_x_inout, CamStart start, int max_iter, double xtol, double lambda0,
                              uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max, void *stream) {
  BA_CHECK(camera_check(who, p, d_x_inout, &max_iter, &xtol, &lambda0));
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)p->stream;
  BA_CHECK(camera_launch(p, d_x_inout, start, nullptr, GEN_LINEAR, max_iter, xtol, lambda0, d_status, d_cost, st));
  return block_counts(p->cams, counts, iters_max, st);
}

static int refine_cameras_host(const char *who, ba_problem *p, double *x_inout, CamStart start, int max_iter, double xtol, double lambda0,
                               uint8_t *status, double *cost, int64_t *counts, int *iters_max) {
  BA_CHECK(camera_check(who, p, x_inout, &max_iter, &xtol, &lambda0));
  // the cameras only: the point part of the caller's x is never written
  return block_host_entry(p, p->cams, x_inout, p->ncams, 9, 3 * p->npnts, status, cost, counts, iters_max,
                          [&](double *dx, uint8_t *d_status, double *d_cost, hipStream_t st) {
                            return camera_launch(p, dx, start, nullptr, GEN_LINEAR, max_iter, xtol, lambda0, d_status, d_cost, st);
                          });
}

extern "C" int ba_refine_cameras_dev(ba_problem *p, double *d_x_inout, int max_iter, double xtol, double lambda0, uint8_t *d_status,
                                     double *d_cost, int64_t *counts, int *iters_max, void *stream) {
  return refine_cameras_dev("ba_refine_cameras_dev", p, d_x_inout, START_X, max_iter, xtol, lambda0, d_status, d_cost, counts, iters_max,
                            stream);
}

extern "C" int ba_refine_cameras(ba_problem *p, double *x_inout, int max_iter, double xtol, double lambda0, uint8_t *status,
                                 double *cost, int64_t *counts, int *iters_max) {
  return refine_cameras_host("ba_refine_cameras", p, x_inout, START_X, max_iter, xtol, lambda0, status, cost, counts, iters_max);
}

extern "C" int ba_resect_cameras_dev(ba_problem *p, double *d_x_inout, int max_iter, double xtol, double lambda0, uint8_t *d_status,
                                     double *d_cost, int64_t *counts, int *iters_max, void *stream) {
  return refine_cameras_dev("ba_resect_cameras_dev", p, d_x_inout, START_RESECT, max_iter, xtol, lambda0, d_status, d_cost, counts, iters_max,
                            stream);
}

extern "C" int ba_resect_cameras(ba_problem *p, double *x_inout, int max_iter, double xtol, double lambda0, uint8_t *status,
                                 double *cost, int64_t *counts, int *iters_max) {
  return refine_cameras_host("ba_resect_cameras", p, x_inout, START_RESECT, max_iter, xtol, lambda0, status, cost, counts, iters_max);
}

extern "C" int ba_resect_cameras_focal_dev(ba_problem *p, double *d_x_inout, int max_iter, double xtol, double lambda0,
                                           uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max, void *stream) {
  return refine_cameras_dev("ba_resect_cameras_focal_dev", p, d_x_inout, START_FOCAL, max_iter, xtol, lambda0, d_status, d_cost, counts,
                            iters_max, stream);
}

extern "C" int ba_resect_cameras_focal(ba_problem *p, double *x_inout, int max_iter, double xtol, double lambda0, uint8_t *status,
                                       double *cost, int64_t *counts, int *iters_max) {
  return refine_cameras_host("ba_resect_cameras_focal", p, x_inout, START_FOCAL, max_iter, xtol, lambda0, status, cost, counts, iters_max);
}

// ---- ba_ransac_cameras: a consensus stage in front of ba_resect_cameras ------------------------------------------
// the consensus results of the last ransac_consensus -> the caller's arrays (each may be null), on st
static int ransac_results(ba_problem *p, uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp, hipMemcpyKind kind, hipStream_t st) {
  const CameraWork &w = p->cams;
  if (p->ncams == 0) return BA_OK;
  if (inlier && p->nobs > 0) BA_HIP_CHECK(hipMemcpyAsync(inlier, w.rs_inlier, (size_t)p->nobs, kind, st));
  if (n_inliers) BA_HIP_CHECK(hipMemcpyAsync(n_inliers, w.rs_n, (size_t)p->ncams * sizeof(int32_t), kind, st));
  if (best_hyp) BA_HIP_CHECK(hipMemcpyAsync(best_hyp, w.rs_best, (size_t)p->ncams * sizeof(int32_t), kind, st));
  return BA_OK;
}

// the options of an entry under its generator: P3P takes samples of exactly 3; the sets are those of the linear resection
static int ransac_cameras_opts(const char *who, RansacGen gen, const ba_ransac_opts *opts, ba_ransac_opts *o) {
  if (gen == GEN_P3P) return ransac_opts_check(who, opts, o, RS_P3P_SAMPLE, RS_MIN_OBS, RS_P3P_SAMPLE);
  return ransac_opts_check(who, opts, o, RS_MIN_OBS);
}

static int ransac_cameras_dev(const char *who, ba_problem *p, double *d_x_inout, CamStart start, RansacGen gen, const ba_ransac_opts *opts, int max_iter,
                              double xtol, double lambda0, uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max,
                              uint8_t *d_inlier, int32_t *d_n_inliers, int32_t *d_best_hyp, void *stream) {
  ba_ransac_opts o;
  BA_CHECK(ransac_cameras_opts(who, gen, opts, &o));
  BA_CHECK(camera_check(who, p, d_x_inout, &max_iter, &xtol, &lambda0));
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)p->stream;
  BA_CHECK(camera_launch(p, d_x_inout, start, &o, gen, max_iter, xtol, lambda0, d_status, d_cost, st));
  BA_CHECK(ransac_results(p, d_inlier, d_n_inliers, d_best_hyp, hipMemcpyDeviceToDevice, st));
  return block_counts(p->cams, counts, iters_max, st);
}

static int ransac_cameras_host(const char *who, ba_problem *p, double *x_inout, CamStart start, RansacGen gen, const ba_ransac_opts *opts, int max_iter,
                               double xtol, double lambda0, uint8_t *status, double *cost, int64_t *counts, int *iters_max,
                               uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp) {
  ba_ransac_opts o;
  BA_CHECK(ransac_cameras_opts(who, gen, opts, &o));
  BA_CHECK(camera_check(who, p, x_inout, &max_iter, &xtol, &lambda0));
  return block_host_entry(p, p->cams, x_inout, p->ncams, 9, 3 * p->npnts, status, cost, counts, iters_max,
                          [&](double *dx, uint8_t *d_status, double *d_cost, hipStream_t st) {
                            BA_CHECK(camera_launch(p, dx, start, &o, gen, max_iter, xtol, lambda0, d_status, d_cost, st));
                            return ransac_results(p, inlier, n_inliers, best_hyp, hipMemcpyDeviceToHost, st);
                          });
}

extern "C" int ba_ransac_cameras_dev(ba_problem *p, double *d_x_inout, const ba_ransac_opts *opts, int max_iter, double xtol,
    double lambda0, uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max, uint8_t *d_inlier, int32_t *d_n_inliers,
    int32_t *d_best_hyp, void *stream) {
  return ransac_cameras_dev("ba_ransac_cameras_dev", p, d_x_inout, START_RESECT, GEN_LINEAR, opts, max_iter, xtol, lambda0, d_status, d_cost, counts, iters_max,
                            d_inlier, d_n_inliers, d_best_hyp, stream);
}

extern "C" int ba_ransac_cameras(ba_problem *p, double *x_inout, const ba_ransac_opts *opts, int max_iter, double xtol, double lambda0,
    uint8_t *status, double *cost, int64_t *counts, int *iters_max, uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp) {
  return ransac_cameras_host("ba_ransac_cameras", p, x_inout, START_RESECT, GEN_LINEAR, opts, max_iter, xtol, lambda0, status, cost, counts, iters_max, inlier,
                             n_inliers, best_hyp);
}

extern "C" int ba_ransac_cameras_focal_dev(ba_problem *p, double *d_x_inout, const ba_ransac_opts *opts, int max_iter, double xtol,
    double lambda0, uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max, uint8_t *d_inlier, int32_t *d_n_inliers,
    int32_t *d_best_hyp, void *stream) {
  return ransac_cameras_dev("ba_ransac_cameras_focal_dev", p, d_x_inout, START_FOCAL, GEN_LINEAR, opts, max_iter, xtol, lambda0, d_status, d_cost, counts, iters_max,
                            d_inlier, d_n_inliers, d_best_hyp, stream);
}

extern "C" int ba_ransac_cameras_focal(ba_problem *p, double *x_inout, const ba_ransac_opts *opts, int max_iter, double xtol, double lambda0,
    uint8_t *status, double *cost, int64_t *counts, int *iters_max, uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp) {
  return ransac_cameras_host("ba_ransac_cameras_focal", p, x_inout, START_FOCAL, GEN_LINEAR, opts, max_iter, xtol, lambda0, status, cost, counts, iters_max, inlier,
                             n_inliers, best_hyp);
}

// ---- ba_ransac_cameras_p3p: the same call with P3P on three correspondences as the hypothesis generator ------------
extern "C" int ba_ransac_cameras_p3p_dev(ba_problem *p, double *d_x_inout, const ba_ransac_opts *opts, int max_iter, double xtol,
    double lambda0, uint8_t *d_status, double *d_cost, int64_t *counts, int *iters_max, uint8_t *d_inlier, int32_t *d_n_inliers,
    int32_t *d_best_hyp, void *stream) {
  return ransac_cameras_dev("ba_ransac_cameras_p3p_dev", p, d_x_inout, START_RESECT, GEN_P3P, opts, max_iter, xtol, lambda0, d_status, d_cost, counts,
                            iters_max, d_inlier, d_n_inliers, d_best_hyp, stream);
}

extern "C" int ba_ransac_cameras_p3p(ba_problem *p, double *x_inout, const ba_ransac_opts *opts, int max_iter, double xtol, double lambda0,
    uint8_t *status, double *cost, int64_t *counts, int *iters_max, uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp) {
  return ransac_cameras_host("ba_ransac_cameras_p3p", p, x_inout, START_RESECT, GEN_P3P, opts, max_iter, xtol, lambda0, status, cost, counts, iters_max,
                             inlier, n_inliers, best_hyp);
}
