// The consensus stage of ba_ransac_cameras (include/ba_hip.h, "outlier-robust camera resection").  gfx950 only.
//
// k_ransac_hypotheses: grid (camera, hypotheses / 4), ONE WAVE PER HYPOTHESIS.  The usual call registers a handful of cameras
// with thousands of correspondences each; one workgroup per camera, as k_resect_cameras has it, would leave the chip empty.
// A wave draws its minimal sample (one draw per lane: the 64 draws of the header at once), takes the 4 + 40 sums of the
// sampled observations through wave_all_sum and then runs the linear resection of ba_refine_dev.h on its own LDS slab (a
// ResectScratch): the very functions k_resect_cameras runs per workgroup, so the same sums give the same pose, bit for bit.
// It counts the inliers of the camera's whole list in a strided pass.  The four waves of a workgroup never meet: the phases of
// a Jacobi rotation are ordered inside the wave (jacobi12<wave_sync>: the LDS operations of one wave complete in order, the
// fence keeps the compiler from moving them), so the kernel has no workgroup barrier and a wave whose sample is void or
// degenerate simply leaves.
// k_ransac_hypotheses_p3p (ba_ransac_cameras_p3p) is the same grid with another generator: three draws, the P3P
// solver of ba_refine_dev.h in every lane's registers, one scoring pass per solution; no LDS.  k_p3p (ba_p3p) runs that solver
// alone, one problem per lane.
// k_ransac_select (one workgroup per camera) picks the winner and writes the inlier bytes; k_ransac_rescore compares the set
// a refit gives with the current one; k_ransac_mask_info hands the set to k_resect_cameras / k_refine_cameras as information.
// All three kernels that test an observation call ransac_inlier, so a count never disagrees with the bytes.
// The rules a consensus call's result hangs on -- which draws are the sample, which hypothesis wins, when a refit's set is
// adopted -- are in ba_consensus_dev.h, shared with ba_relative_pose; this file keeps the geometry of a hypothesis
// (hypothesis_pose from the sums onward), the inlier test and the branch of a camera that is not attempted.  The check of the
// options of both entries (ransac_opts_check), ba_ransac_sample and ba_p3p are at the end of the file.
// No floating-point atomics, no integer ones either: every output has one writer.
// Focal mode (RansacArgs.focal and the camera's f free; ba_ransac_cameras_focal): a hypothesis estimates f from its
// own eigenvector and is scored under it -- its record carries that f, and the refits leave theirs in the scratch cameras.
#include <cmath>

#include "ba_internal.h"

// (ransac_mix, ransac_draw, RN_DRAWS and the limits of the options -- splitmix64, the one generator of the sampling, host and
// device -- are in ba_internal.h)

namespace {

#include "ba_model_dev.h"      // cam_pre, project_pre
#include "ba_refine_dev.h"     // wave_all_sum, p1_z, obs_used, the pieces of the linear resection
#include "ba_consensus_dev.h"  // the sample, the winner, the set and the adopt rule: shared with ba_pair_kernels.hip

constexpr int RN_BLK = CS_BLK, RN_WAVES = CS_WAVES;

// the inlier test of the header under the cam_pre row P: used, in front (P1.z < 0), within tau of its measurement in raw pixels
// (a comparison with NaN fails)
__device__ __forceinline__ bool ransac_inlier(const RansacArgs &a, const double P[12], int o) {
  if (!obs_used(a.info, o)) return false;
  const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
  const double X[3] = {xp[0], xp[1], xp[2]};
  const double2 m = reinterpret_cast<const double2 *>(a.pt2d)[o];
  double out[2], z1;
  project_pre<double>(X, P, out);
  p1_z(P, X, z1);
  const double ex = out[0] - m.x, ey = out[1] - m.y;
  return z1 < 0.0 && ex * ex + ey * ey <= a.tau2;
}

// cam_pre row of the camera (pose, k1, k2, f)
__device__ __forceinline__ void pose_row(const double *pose, double k1, double k2, double f, double P[12]) {
  const double C9[9] = {pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], k1, k2, f};
  cam_pre<double>(C9, P);
}

// (k1, k2) a camera's hypotheses are undistorted with and scored under: those of xc; in focal mode, where nothing is undistorted,
// a held one from xc and 0 for a free one (which is never read)
__device__ __forceinline__ void scoring_distortion(const double *xc, bool focal, unsigned fm, double &k1, double &k2) {
  k1 = (focal && !(fm & K1_HELD)) ? 0.0 : xc[6];
  k2 = (focal && !(fm & K2_HELD)) ? 0.0 : xc[7];
}

// The pose of hypothesis h of camera c (list [k0, k1), intrinsics xc[6..8], mask fm) -> its cam_pre row P and pose[7]: r, t and
// the f it is scored under -- that of xc, or in focal mode the estimate from the sample's own eigenvector; false:
// void (too few distinct used draws) or degenerate.  Called by a whole wave; the control flow is uniform over it.
__device__ __forceinline__ bool hypothesis_pose(const RansacArgs &a, ResectScratch &sh, const double *xc, bool focal, unsigned fm, int h,
                                                int k0, int k1, int lane, double pose[RANSAC_HYP_DOUBLES], double P[12]) {
  const int d = k1 - k0, m = a.sample;
  double ck1, ck2, cf = xc[8];  // (focal mode: cf is not used until the image scale takes its place)
  scoring_distortion(xc, focal, fm, ck1, ck2);
  if (d <= 0 || (!focal && (!isfinite(cf) || cf == 0.0))) return false;
  // the sample: lane j holds draw j
  const int pos = sample_position(a.seed_mix, h, lane, d), o = a.cam_obs[k0 + pos];
  bool take;
  int first;
  if (!sample_take(pos, obs_used(a.info, o), lane, m, take, first)) return false;
  double X[3] = {0.0, 0.0, 0.0}, mx = 0.0, my = 0.0;
  if (take) {
    const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
    X[0] = xp[0], X[1] = xp[1], X[2] = xp[2];
    const double2 mm = reinterpret_cast<const double2 *>(a.pt2d)[o];
    mx = mm.x, my = mm.y;
  }
  const double org[3] = {__shfl(X[0], first, 64), __shfl(X[1], first, 64), __shfl(X[2], first, 64)};
  // the mean of the sampled points and their RMS distance from it
  double mo[4] = {0, 0, 0, 0};
  if (take) {
    const double d0 = X[0] - org[0], d1 = X[1] - org[1], d2 = X[2] - org[2];
    mo[0] = d0, mo[1] = d1, mo[2] = d2;
    mo[3] = (d0 * d0 + d1 * d1) + d2 * d2;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) mo[i] = wave_all_sum(mo[i]);
  double dm[3], sc;
  if (!hartley_stats((double)m, mo, mo[3], dm, sc)) return false;
  if (focal && !image_scale((double)m, wave_all_sum(mx * mx + my * my), cf)) return false;
  // the moments: a lane that takes no draw adds zeros
  double hh[4] = {0.0, 0.0, 0.0, 0.0}, qx = 0.0, qy = 0.0, acc[RS_SUMS];
  if (take) {
    normalised_point(X, org, dm, sc, hh);
    if (focal) qx = mx / cf, qy = my / cf;
    else undistort(mx / cf, my / cf, ck1, ck2, qx, qy);
  }
  moment_terms(hh, qx, qy, acc);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < RS_SUMS; i++) {
    acc[i] = wave_all_sum(acc[i]);
    ok = ok && isfinite(acc[i]);
  }
  if (!ok) return false;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < RS_SUMS; i++) sh.S[i] = acc[i];
  }
  wave_sync();
  for (int e = lane; e < 144; e += 64) sh.M[e] = normal_matrix_entry(sh.S, e);
  jacobi12<wave_sync>(sh.M, sh.V, lane, 64);
  int i1;
  if (!smallest_eigenpair(sh.M, i1)) return false;
  // the points of the sample in front of the camera under the eigenvector's sign
  const int front = __popcll(__ballot(take && front_z(sh.V, i1, hh) < 0.0));
  if (lane == 0) {
    const double sgn = 2 * front >= m ? 1.0 : -1.0;
    sh.ok = ((!focal || focal_from_eigenvector(sh, i1, cf)) && pose_from_eigenvector(sh, i1, sgn, sc, org, dm)) ? 1 : 0;
  }
  wave_sync();
  if (!sh.ok) return false;
  pose[0] = sh.r[0], pose[1] = sh.r[1], pose[2] = sh.r[2];
  pose[3] = sh.tr[0], pose[4] = sh.tr[1], pose[5] = sh.tr[2];
  pose[6] = focal ? sh.f : cf;
  pose_row(pose, ck1, ck2, pose[6], P);
  return true;
}

__global__ __launch_bounds__(RN_BLK) void k_ransac_hypotheses(RansacArgs a) {
  __shared__ ResectScratch shs[RN_WAVES];  // one wave's slab each
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int c = (int)blockIdx.x, h = (int)blockIdx.y * RN_WAVES + wv;
  if (h >= a.hypotheses) return;
  const unsigned fm = a.mask ? (unsigned)a.mask[c] : 0u;
  if (fm & POSE_MASK) return;  // not attempted: k_ransac_select reads nothing of it
  const int k0 = a.cam_ptr[c], k1 = a.cam_ptr[c + 1];
  const int64_t slot = (int64_t)c * a.hypotheses + h;
  double pose[RANSAC_HYP_DOUBLES], P[12];
  int count = -1;
  if (hypothesis_pose(a, shs[wv], a.xc + 9 * (int64_t)c, focal_mode(a.focal, fm), fm, h, k0, k1, lane, pose, P)) {
    count = 0;
    for (int k = k0 + lane; k < k1; k += 64) count += ransac_inlier(a, P, a.cam_obs[k]) ? 1 : 0;
    count = wave_all_sum_int(count);
  }
  if (lane == 0) {
    a.hyp_count[slot] = count;
    if (count >= 0) {
#pragma unroll
      for (int i = 0; i < RANSAC_HYP_DOUBLES; i++) a.hyp_pose[RANSAC_HYP_DOUBLES * slot + i] = pose[i];
    }
  }
}

// Hypothesis h of a camera from the P3P solver (ba_ransac_cameras_p3p), the grid and the layout of
// k_ransac_hypotheses: the wave draws three correspondences, every lane takes all three (shuffles from the lanes of the draws)
// and runs p3p_solve on them in its own registers -- 64 times the same bits, which costs the time of one and needs neither LDS
// nor an exchange -- and every solution is scored in one strided pass over the camera's list.  The hypothesis is the solution
// with the largest count, ties to the first in ascending order of the quartic's root; no sample, no solution: void.  The
// intrinsics are those of x; there is no focal mode.
__global__ __launch_bounds__(RN_BLK) void k_ransac_hypotheses_p3p(RansacArgs a) {
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int c = (int)blockIdx.x, h = (int)blockIdx.y * RN_WAVES + wv;
  if (h >= a.hypotheses) return;
  const unsigned fm = a.mask ? (unsigned)a.mask[c] : 0u;
  if (fm & POSE_MASK) return;  // not attempted: k_ransac_select reads nothing of it
  const int k0 = a.cam_ptr[c], k1 = a.cam_ptr[c + 1], d = k1 - k0;
  const int64_t slot = (int64_t)c * a.hypotheses + h;
  const double *xc = a.xc + 9 * (int64_t)c;
  const double ck1 = xc[6], ck2 = xc[7], cf = xc[8];
  int best = -1;
  double keep[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (d > 0 && isfinite(cf) && cf != 0.0) {
    const int pos = sample_position(a.seed_mix, h, lane, d), o = a.cam_obs[k0 + pos];
    bool take;
    int first;
    if (sample_take(pos, obs_used(a.info, o), lane, P3_POINTS, take, first)) {
      double Xl[3] = {0.0, 0.0, 0.0}, qx = 0.0, qy = 0.0;
      if (take) {
        const double *xp = a.x + 3 * (int64_t)a.pnt0[o];
        Xl[0] = xp[0], Xl[1] = xp[1], Xl[2] = xp[2];
        const double2 mm = reinterpret_cast<const double2 *>(a.pt2d)[o];
        undistort(mm.x / cf, mm.y / cf, ck1, ck2, qx, qy);
      }
      unsigned long long from = __ballot(take);  // the lanes of the three draws, in their order
      double q[P3_POINTS][2], X[P3_POINTS][3];
#pragma unroll
      for (int i = 0; i < P3_POINTS; i++) {
        const int l = __ffsll((long long)from) - 1;
        from &= from - 1ull;
        q[i][0] = __shfl(qx, l, 64), q[i][1] = __shfl(qy, l, 64);
        X[i][0] = __shfl(Xl[0], l, 64), X[i][1] = __shfl(Xl[1], l, 64), X[i][2] = __shfl(Xl[2], l, 64);
      }
      double pose[P3_MAX_SOL][6];
      const unsigned found = p3p_solve(q, X, pose);  // (uniform over the wave)
#pragma unroll
      for (int s = 0; s < P3_MAX_SOL; s++) {
        if (!((found >> s) & 1u)) continue;
        double P[12];
        pose_row(pose[s], ck1, ck2, cf, P);
        int count = 0;
        for (int k = k0 + lane; k < k1; k += 64) count += ransac_inlier(a, P, a.cam_obs[k]) ? 1 : 0;
        count = wave_all_sum_int(count);
        if (count > best) {
          best = count;
#pragma unroll
          for (int i = 0; i < 6; i++) keep[i] = pose[s][i];
        }
      }
    }
  }
  if (lane == 0) {
    a.hyp_count[slot] = best;
    if (best >= 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) a.hyp_pose[RANSAC_HYP_DOUBLES * slot + i] = keep[i];
      a.hyp_pose[RANSAC_HYP_DOUBLES * slot + 6] = cf;
    }
  }
}

// ba_p3p: one problem per lane (p3p_solve is one lane's work, as in the hypothesis kernel); pose: 4 x 6 per problem, the
// solutions first, the unused slots NaN
__global__ __launch_bounds__(RN_BLK) void k_p3p(int64_t n, const double *q, const double *X, double *pose, int *n_sol) {
  const int64_t i = (int64_t)blockIdx.x * RN_BLK + threadIdx.x;
  if (i >= n) return;
  double ql[P3_POINTS][2], Xl[P3_POINTS][3], sol[P3_MAX_SOL][6];
#pragma unroll
  for (int k = 0; k < P3_POINTS; k++) {
    ql[k][0] = q[6 * i + 2 * k], ql[k][1] = q[6 * i + 2 * k + 1];
    Xl[k][0] = X[9 * i + 3 * k], Xl[k][1] = X[9 * i + 3 * k + 1], Xl[k][2] = X[9 * i + 3 * k + 2];
  }
  const unsigned found = p3p_solve(ql, Xl, sol);
  double *out = pose + 6 * P3_MAX_SOL * i;
  int ns = 0;
#pragma unroll
  for (int s = 0; s < P3_MAX_SOL; s++) {
    if (!((found >> s) & 1u)) continue;
#pragma unroll
    for (int e = 0; e < 6; e++) out[6 * ns + e] = sol[s][e];
    ns++;
  }
  for (int e = 6 * ns; e < 6 * P3_MAX_SOL; e++) out[e] = __longlong_as_double(0x7ff8000000000000ll);
  n_sol[i] = ns;
}

// One camera per workgroup: the winner among its hypotheses (consensus_winner), its inlier bytes, the size of the set, the
// winner's index and the "stopped" byte.  A camera that is not attempted: its used observations, -1, stopped.
__global__ __launch_bounds__(RN_BLK) void k_ransac_select(RansacArgs a) {
  __shared__ long long redk[RN_WAVES];
  __shared__ int red[RN_WAVES];
  const int t = (int)threadIdx.x, c = (int)blockIdx.x;
  const int k0 = a.cam_ptr[c], k1 = a.cam_ptr[c + 1];
  const unsigned fm = a.mask ? (unsigned)a.mask[c] : 0u;
  const auto obs_of = [&](int k) { return a.cam_obs[k]; };
  if (fm & POSE_MASK) {
    const int n = consensus_mark(k0, k1, a.inlier, red, t, obs_of, [&](int o) { return obs_used(a.info, o); });
    if (t == 0) a.n_inliers[c] = n, a.best_hyp[c] = -1, a.stopped[c] = 1;
    return;
  }
  int best, best_count;
  consensus_winner(a.hyp_count + (int64_t)c * a.hypotheses, a.hypotheses, t, redk, best, best_count);
  if (best < 0 || best_count < a.min_inliers) {  // the camera fails: no inlier, the finish finds it DEGENERATE
    for (int k = k0 + t; k < k1; k += RN_BLK) a.inlier[a.cam_obs[k]] = 0;
    if (t == 0) a.n_inliers[c] = best_count, a.best_hyp[c] = best, a.stopped[c] = 1;
    return;
  }
  double P[12], ck1, ck2;  // the winner's row: its pose and the f it was scored under
  const double *win = a.hyp_pose + RANSAC_HYP_DOUBLES * ((int64_t)c * a.hypotheses + best);
  scoring_distortion(a.xc + 9 * (int64_t)c, focal_mode(a.focal, fm), fm, ck1, ck2);
  pose_row(win, ck1, ck2, win[6], P);
  const int n = consensus_mark(k0, k1, a.inlier, red, t, obs_of, [&](int o) { return ransac_inlier(a, P, o); });
  if (t == 0) a.n_inliers[c] = n, a.best_hyp[c] = best, a.stopped[c] = 0;
}

// One camera per workgroup, after a refit on its set M wrote a pose into cams (the scratch copy of the cameras: its intrinsics
// are those of x, or in focal mode what the refit wrote): the adopt rule of consensus_rescore on the whole list under that
// camera; M stays and the camera stops when M' is not adopted, and when the refit found no pose.
__global__ __launch_bounds__(RN_BLK) void k_ransac_rescore(RansacArgs a, const double *cams, const uint8_t *resect) {
  __shared__ int red[RN_WAVES];
  const int t = (int)threadIdx.x, c = (int)blockIdx.x;
  if (a.stopped[c]) return;
  if (resect[c] == 2) {  // (RS_DEGENERATE of k_resect_cameras)
    if (t == 0) a.stopped[c] = 1;
    return;
  }
  const int k0 = a.cam_ptr[c], k1 = a.cam_ptr[c + 1];
  const int n_old = a.n_inliers[c];
  double P[12];
  const double *cam = cams + 9 * (int64_t)c;
  pose_row(cam, cam[6], cam[7], cam[8], P);
  const int n = consensus_rescore(
      k0, k1, n_old, a.inlier, red, t, [&](int k) { return a.cam_obs[k]; }, [&](int o) { return ransac_inlier(a, P, o); });
  if (t == 0) {
    if (n >= 0) a.n_inliers[c] = n;
    else a.stopped[c] = 1;
  }
}

__global__ __launch_bounds__(RN_BLK) void k_ransac_mask_info(RansacArgs a, int64_t nobs, double *out) {
  const int64_t o = (int64_t)blockIdx.x * RN_BLK + threadIdx.x;
  if (o >= nobs) return;
  double l00 = 0.0, l10 = 0.0, l11 = 0.0;
  if (a.inlier[o] & 1) {
    if (a.info) l00 = a.info[3 * o], l10 = a.info[3 * o + 1], l11 = a.info[3 * o + 2];
    else l00 = 1.0, l11 = 1.0;
  }
  out[3 * o] = l00, out[3 * o + 1] = l10, out[3 * o + 2] = l11;
}

}  // namespace

uint64_t ransac_seed_mix(uint64_t seed) { return ransac_mix(seed); }

int launch_ransac_hypotheses(const RansacArgs &a, int64_t ncams, RansacGen gen, hipStream_t st) {
  const dim3 grid((unsigned)ncams, grid_for(a.hypotheses, RN_WAVES));
  if (gen == GEN_P3P) return BA_LAUNCH(k_ransac_hypotheses_p3p, grid, RN_BLK, 0, st, a);
  return BA_LAUNCH(k_ransac_hypotheses, grid, RN_BLK, 0, st, a);
}

int launch_ransac_select(const RansacArgs &a, int64_t ncams, hipStream_t st) {
  return BA_LAUNCH(k_ransac_select, (unsigned)ncams, RN_BLK, 0, st, a);
}

int launch_ransac_rescore(const RansacArgs &a, int64_t ncams, const double *cams, const uint8_t *resect, hipStream_t st) {
  return BA_LAUNCH(k_ransac_rescore, (unsigned)ncams, RN_BLK, 0, st, a, cams, resect);
}

int launch_ransac_mask_info(const RansacArgs &a, int64_t nobs, double *out, hipStream_t st) {
  return BA_LAUNCH(k_ransac_mask_info, grid_for(nobs, RN_BLK), RN_BLK, 0, st, a, nobs, out);
}

int ransac_opts_check(const char *who, const ba_ransac_opts *in, ba_ransac_opts *o, int least, int least_set, int most) {
  if (least_set <= 0) least_set = least;
  if (most <= 0) most = RN_SAMPLE_MAX;
  if (!in) {
    ba_set_error("%s: null options", who);
    return BA_ERR_ARG;
  }
  *o = *in;
  if (!std::isfinite(o->threshold) || !(o->threshold > 0)) {
    ba_set_error("%s: threshold must be finite and > 0 (pixels), got %g", who, o->threshold);
    return BA_ERR_ARG;
  }
  if (o->hypotheses <= 0) o->hypotheses = 128;
  if (o->sample <= 0) o->sample = least;
  if (o->refits < 0) o->refits = 2;
  if (o->hypotheses > RN_HYP_MAX || o->sample < least || o->sample > most || o->refits > RN_REFITS_MAX) {
    if (least == most)
      ba_set_error("%s: hypotheses must be <= %d, sample must be %d, refits <= %d, got %d, %d, %d", who, RN_HYP_MAX, least, RN_REFITS_MAX,
                   o->hypotheses, o->sample, o->refits);
    else
      ba_set_error("%s: hypotheses must be <= %d, sample in %d..%d, refits <= %d, got %d, %d, %d", who, RN_HYP_MAX, least, most,
                   RN_REFITS_MAX, o->hypotheses, o->sample, o->refits);
    return BA_ERR_ARG;
  }
  if (o->min_inliers <= 0) o->min_inliers = o->sample > least_set ? o->sample : least_set;  // (>= least_set)
  if (o->min_inliers < least_set) {
    ba_set_error("%s: min_inliers must be >= %d (<= 0: max(sample, %d)), got %d", who, least_set, least_set, o->min_inliers);
    return BA_ERR_ARG;
  }
  return BA_OK;
}

// the sampling alone, on the host (no device is touched)
extern "C" int ba_ransac_sample(uint64_t seed, int hypothesis, int64_t degree, const uint8_t *used, int sample, int64_t *pos,
                                int *n_taken) {
  if (sample <= 0) sample = RS_MIN_OBS;
  if (!pos || !n_taken || hypothesis < 0 || degree < 0 || degree > (int64_t)INT32_MAX || sample < RS_MIN_OBS || sample > RN_SAMPLE_MAX) {
    ba_set_error("ba_ransac_sample: null argument, hypothesis < 0, degree outside 0..2^31 - 1 or sample outside %d..%d", RS_MIN_OBS,
                 RN_SAMPLE_MAX);
    return BA_ERR_ARG;
  }
  const uint64_t key = ransac_mix(ransac_mix(seed) ^ (uint64_t)hypothesis);
  int n = 0;
  for (int j = 0; j < RN_DRAWS && n < sample && degree > 0; j++) {
    const int64_t q = ransac_draw(key, j, degree);
    bool skip = used && !used[q];
    for (int i = 0; i < n; i++) skip = skip || pos[i] == q;
    if (!skip) pos[n++] = q;
  }
  *n_taken = n;
  return BA_OK;
}

// the P3P solver alone; the handle supplies the device, the stream and the buffers
extern "C" int ba_p3p(ba_problem *p, int64_t n, const double *q, const double *X, double *pose, int32_t *n_sol) {
  if (!p || n < 0 || (n > 0 && (!q || !X || !pose || !n_sol))) {
    ba_set_error("ba_p3p: null argument or n < 0");
    return BA_ERR_ARG;
  }
  if (n > (int64_t)INT32_MAX / (6 * P3_MAX_SOL)) {
    ba_set_error("ba_p3p: %lld problems: more than %lld", (long long)n, (long long)(INT32_MAX / (6 * P3_MAX_SOL)));
    return BA_ERR_ARG;
  }
  if (n == 0) return BA_OK;
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  CameraWork &w = p->cams;
  if (w.p3_cap < n) {
    w.p3_cap = 0;
    BA_CHECK(w.p3_q.alloc(2 * P3_POINTS * n));
    BA_CHECK(w.p3_X.alloc(3 * P3_POINTS * n));
    BA_CHECK(w.p3_pose.alloc(6 * P3_MAX_SOL * n));
    BA_CHECK(w.p3_n.alloc(n));
    w.p3_cap = n;
  }
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.p3_q, q, (size_t)(2 * P3_POINTS * n) * sizeof(double), hipMemcpyHostToDevice, st));
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.p3_X, X, (size_t)(3 * P3_POINTS * n) * sizeof(double), hipMemcpyHostToDevice, st));
  {
    ProfScope ps(p, PC_RANSAC_CAMERAS, st);  // (the class of the consensus kernels: the solver is their generator)
    BA_CHECK(BA_LAUNCH(k_p3p, grid_for(n, RN_BLK), RN_BLK, 0, st, n, w.p3_q, w.p3_X, w.p3_pose, w.p3_n));
  }
  BA_HIP_CHECK(hipMemcpyAsync(pose, w.p3_pose, (size_t)(6 * P3_MAX_SOL * n) * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(n_sol, w.p3_n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}
