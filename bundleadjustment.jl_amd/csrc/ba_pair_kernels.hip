// Two-view relative pose (ba_pair_matches, ba_relative_pose, ba_relative_pose_five_point, ba_five_point, ba_refine_relative_pose; include/ba_hip.h, "relative pose of camera pairs").
// gfx950 only.
//
// The host lists the matches of every pair (pair_match_lists: the points both cameras observe, ordered by camera a's list) and
// uploads them with the six intrinsics of the pair; the poses and points of x never reach the device.
// k_pair_rays: one lane per match undistorts both measurements ONCE into a 40-byte record (q_a, q_b, used): the H hypotheses of
// a pair read that record and never repeat the 16 divisions per match.
// k_pair_hypotheses: grid (pair, hypotheses / 4), ONE WAVE PER HYPOTHESIS on its own LDS slab (a PairScratch), the layout of
// k_ransac_hypotheses: a wave draws its sample (one draw per lane), takes the 6 + 45 sums through wave_all_sum, runs the linear
// fit of ba_refine_dev.h (essential_from_sums<wave_sync>: no workgroup barrier, a void or degenerate wave simply leaves) and
// counts the inliers of the pair's whole list in a strided pass over the records.
// k_pair_hypotheses5 (ba_relative_pose_five_point): the same layout with the five-point solver of ba_refine_dev.h as the
// generator: every real essential matrix through five sampled matches is scored, the best is the hypothesis.  k_five_point
// (ba_five_point) runs that solver alone, one wave per tuple.
// k_pair_select (one workgroup per pair): the states that need no fit, the winner, its inlier bytes.
// k_pair_fit (one workgroup per pair): the sums over the current set in a fixed order (strided partial sums per thread, the
// butterfly of a wave, the four waves in order), the same linear fit (essential_from_sums<__syncthreads>), then either the
// re-scoring with the adopt rule of the refits or, in the last launch, the returned pose.
// k_pair_refine (ba_refine_relative_pose; one workgroup per pair, the layout of k_pair_fit): the Marquardt iteration
// on the Sampson error of the pair's set, the whole loop of a round in one launch -- the 21 sums of a trial in the same fixed
// order, the 5 x 5 Cholesky and the retraction by one thread in LDS -- then the list re-scored under the refined pose.
// The sample, the winner, the marking of a set and the adopt rule are those of ba_consensus_dev.h, shared with
// ba_ransac_cameras, and the options go through its ransac_opts_check; this file keeps whether a match is used, the sums of a
// fit, the cheirality counts and the states of k_pair_select.
// All kernels that test a match call pair_inlier, so a count never disagrees with the bytes.  No atomics: every output has one
// writer, two calls give the same bits.
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"  // info_upload

namespace {

#include "ba_refine_dev.h"     // wave_all_sum, undistort, obs_used, jacobi12, the pieces of the linear fit
#include "ba_consensus_dev.h"  // the sample, the winner, the set and the adopt rule: shared with ba_ransac_kernels.hip

constexpr int PR_BLK = CS_BLK, PR_WAVES = CS_WAVES;

__global__ __launch_bounds__(PR_BLK) void k_pair_rays(PairArgs a, int64_t nmatch) {
  const int64_t k = (int64_t)blockIdx.x * PR_BLK + threadIdx.x;
  if (k >= nmatch) return;
  const double *in = a.intr + 6 * (int64_t)a.pair_of[k];
  const int oa = a.obs_a[k], ob = a.obs_b[k];
  const double2 ma = reinterpret_cast<const double2 *>(a.pt2d)[oa], mb = reinterpret_cast<const double2 *>(a.pt2d)[ob];
  double *ray = a.rays + PAIR_RAY * k;
  double qx, qy;
  undistort(ma.x / in[2], ma.y / in[2], in[0], in[1], qx, qy);
  ray[0] = qx, ray[1] = qy;
  undistort(mb.x / in[5], mb.y / in[5], in[3], in[4], qx, qy);
  ray[2] = qx, ray[3] = qy;
  ray[4] = (obs_used(a.info, oa) && obs_used(a.info, ob)) ? 1.0 : 0.0;
}

// The linear fit of hypothesis h of a pair (matches [k0, k1), intrinsics in) -> sh.rs.r, sh.t; false: void (too few distinct used
// draws) or degenerate.  Called by a whole wave; the control flow is uniform over it.
__device__ __forceinline__ bool pair_hypothesis(const PairArgs &a, PairScratch &sh, const double *in, int h, int k0, int k1, int lane) {
  const int d = k1 - k0, m = a.sample;
  if (d <= 0 || !pair_focals_ok(in)) return false;
  // the sample: lane j holds draw j
  const int pos = sample_position(a.seed_mix, h, lane, d);
  const double *ray = a.rays + PAIR_RAY * (int64_t)(k0 + pos);
  bool take;
  int first;
  if (!sample_take(pos, ray[4] != 0.0, lane, m, take, first)) return false;
  double qax = 0.0, qay = 0.0, qbx = 0.0, qby = 0.0;
  if (take) qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
  const double oa[2] = {__shfl(qax, first, 64), __shfl(qay, first, 64)}, ob[2] = {__shfl(qbx, first, 64), __shfl(qby, first, 64)};
  // the mean of each image's points and their RMS distance from it
  double mo[6] = {0, 0, 0, 0, 0, 0};
  if (take) {
    const double ax = qax - oa[0], ay = qay - oa[1], bx = qbx - ob[0], by = qby - ob[1];
    mo[0] = ax, mo[1] = ay, mo[2] = ax * ax + ay * ay;
    mo[3] = bx, mo[4] = by, mo[5] = bx * bx + by * by;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) mo[i] = wave_all_sum(mo[i]);
  double dma[3], dmb[3], sa, sb;
  if (!image_stats((double)m, mo[0], mo[1], mo[2], dma, sa) || !image_stats((double)m, mo[3], mo[4], mo[5], dmb, sb)) return false;
  // the 45 sums: a lane that takes no draw adds zeros
  double da[3] = {0.0, 0.0, 0.0}, db[3] = {0.0, 0.0, 0.0}, acc[EP_SUMS];
  if (take) {
    normalised_ray(qax, qay, oa, dma, sa, da);
    normalised_ray(qbx, qby, ob, dmb, sb, db);
  }
  epipolar_terms(da, db, acc);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < EP_SUMS; i++) {
    acc[i] = wave_all_sum(acc[i]);
    ok = ok && isfinite(acc[i]);
  }
  if (!ok) return false;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < EP_SUMS; i++) sh.S[i] = acc[i];
  }
  wave_sync();
  const double ca[2] = {oa[0] + dma[0], oa[1] + dma[1]}, cb[2] = {ob[0] + dmb[0], ob[1] + dmb[1]};
  if (!essential_from_sums<wave_sync>(sh, lane, 64, ca, sa, cb, sb)) return false;
  // the matches of the sample in front of both cameras, per candidate
  int cnt[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    double al, be;
    pair_depths(sh.Rc + 9 * (c >> 1), sh.tn, (c & 1) ? -1.0 : 1.0, qax, qay, qbx, qby, al, be);
    cnt[c] = __popcll(__ballot(take && al > 0.0 && be > 0.0));
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; c++) sh.cnt[c] = cnt[c];
    sh.ok = pair_pose_winner(sh) ? 1 : 0;
  }
  wave_sync();
  return sh.ok != 0;
}

__global__ __launch_bounds__(PR_BLK) void k_pair_hypotheses(PairArgs a) {
  __shared__ PairScratch shs[PR_WAVES];  // one wave's slab each
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int pr = (int)blockIdx.x, h = (int)blockIdx.y * PR_WAVES + wv;
  if (h >= a.hypotheses) return;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  const int64_t slot = (int64_t)pr * a.hypotheses + h;
  PairScratch &sh = shs[wv];
  int count = -1;
  if (pair_hypothesis(a, sh, in, h, k0, k1, lane)) {
    PairPose P;
    pair_pose_of(sh.rs.r, sh.t, P);
    count = 0;
    for (int k = k0 + lane; k < k1; k += 64) count += pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2) ? 1 : 0;
    count = wave_all_sum_int(count);
    if (lane < 3) {
      a.hyp_pose[PAIR_HYP_DOUBLES * slot + lane] = sh.rs.r[lane];
      a.hyp_pose[PAIR_HYP_DOUBLES * slot + 3 + lane] = sh.t[lane];
    }
  }
  if (lane == 0) a.hyp_count[slot] = count;
}

// the LDS of one wave of the five-point kernels: the fit's scratch (the null space goes through its 12 x 12) and the solver's
struct FiveSlab {
  PairScratch ps;
  FiveScratch fs;
};

// Hypothesis h of a pair from the five-point solver (ba_relative_pose_five_point), the layout of k_pair_hypotheses:
// the wave draws five matches, solves for the essential matrices through them (five_point_solve) and takes every real solution
// through the second half of the eight-point fit -- the SVD, the four candidates, the cheirality vote over the five, the rotation
// vector -- and through one strided pass over the pair's records.  The hypothesis is the solution with the largest count, ties to
// the one found first; no sample, no solution or no solution with a match in front: void.
__global__ __launch_bounds__(PR_BLK) void k_pair_hypotheses5(PairArgs a) {
  __shared__ FiveSlab shs[PR_WAVES];  // one wave's slab each
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int pr = (int)blockIdx.x, h = (int)blockIdx.y * PR_WAVES + wv;
  if (h >= a.hypotheses) return;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  const int64_t slot = (int64_t)pr * a.hypotheses + h;
  PairScratch &sh = shs[wv].ps;
  FiveScratch &fs = shs[wv].fs;
  const int d = k1 - k0;
  int best = -1;
  double keep = 0.0;  // lanes 0..2: r of the best solution so far, lanes 3..5: its t
  bool take = false;
  int first = 0;
  const int pos = d > 0 ? sample_position(a.seed_mix, h, lane, d) : 0;
  const double *ray = a.rays + PAIR_RAY * (int64_t)(k0 + pos);
  if (d > 0 && pair_focals_ok(in) && sample_take(pos, ray[4] != 0.0, lane, FP_POINTS, take, first)) {
    double qax = 0.0, qay = 0.0, qbx = 0.0, qby = 0.0, da[3] = {0.0, 0.0, 0.0}, db[3] = {0.0, 0.0, 0.0};
    if (take) {
      qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
      da[0] = qax, da[1] = qay, da[2] = -1.0, db[0] = qbx, db[1] = qby, db[2] = -1.0;
    }
    const int n_sol = five_point_solve(sh, fs, da, db, lane);
#pragma nounroll
    for (int s = 0; s < n_sol; s++) {
      if (lane == 0) {
        for (int e = 0; e < 9; e++) sh.rs.W[e] = fs.E[9 * s + e];
        essential_decompose(sh);
      }
      wave_sync();
      int cnt[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        double al, be;
        pair_depths(sh.Rc + 9 * (c >> 1), sh.tn, (c & 1) ? -1.0 : 1.0, qax, qay, qbx, qby, al, be);
        cnt[c] = __popcll(__ballot(take && al > 0.0 && be > 0.0));
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) sh.cnt[c] = cnt[c];
        sh.ok = pair_pose_winner(sh) ? 1 : 0;
      }
      wave_sync();
      if (sh.ok != 0) {
        PairPose P;
        pair_pose_of(sh.rs.r, sh.t, P);
        int count = 0;
        for (int k = k0 + lane; k < k1; k += 64) count += pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2) ? 1 : 0;
        count = wave_all_sum_int(count);
        if (count > best) {
          best = count;
          if (lane < 3) keep = sh.rs.r[lane];
          else if (lane < 6) keep = sh.t[lane - 3];
        }
      }
      wave_sync();  // (lane 0 writes the next solution over what the wave has read)
    }
  }
  if (best >= 0 && lane < PAIR_HYP_DOUBLES) a.hyp_pose[PAIR_HYP_DOUBLES * slot + lane] = keep;
  if (lane == 0) a.hyp_count[slot] = best;
}

// ba_five_point: one wave per tuple, lane j < 5 holds match j; E: 10 x 9 per tuple, the unused slots NaN
__global__ __launch_bounds__(PR_BLK) void k_five_point(int64_t n, const double *qa, const double *qb, double *E, int *n_sol) {
  __shared__ FiveSlab shs[PR_WAVES];
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * PR_WAVES + wv;
  if (i >= n) return;
  double da[3] = {0.0, 0.0, 0.0}, db[3] = {0.0, 0.0, 0.0};
  if (lane < FP_POINTS) {
    const int64_t at = 2 * (FP_POINTS * i + lane);
    da[0] = qa[at], da[1] = qa[at + 1], da[2] = -1.0, db[0] = qb[at], db[1] = qb[at + 1], db[2] = -1.0;
  }
  const int ns = five_point_solve(shs[wv].ps, shs[wv].fs, da, db, lane);
  for (int e = lane; e < 9 * FP_MAX_SOL; e += 64) E[9 * FP_MAX_SOL * i + e] = e < 9 * ns ? shs[wv].fs.E[e] : __longlong_as_double(0x7ff8000000000000ll);
  if (lane == 0) n_sol[i] = ns;
}

// a pair that ends here: its state, no inlier, n matches counted, winner h (or -1)
__device__ __forceinline__ void pair_fails(const PairArgs &a, int pr, int k0, int k1, int t, int state, int n, int h) {
  for (int k = k0 + t; k < k1; k += PR_BLK) a.inlier[k] = 0;
  if (t == 0) a.status[pr] = (uint8_t)state, a.n_inliers[pr] = n, a.best_hyp[pr] = h, a.stopped[pr] = 1;
}

// One pair per workgroup: FEW_MATCHES (fewer than 8 used matches), DEGENERATE (a focal length that is not finite or 0), without
// a consensus stage the set of the used matches, with one the winner among the hypotheses (consensus_winner; none, or a count
// below min_inliers: NO_CONSENSUS) and its inlier bytes.
__global__ __launch_bounds__(PR_BLK) void k_pair_select(PairArgs a) {
  __shared__ long long redk[PR_WAVES];
  __shared__ int red[PR_WAVES];
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  int nu = 0;
  for (int k = k0 + t; k < k1; k += PR_BLK) nu += a.rays[PAIR_RAY * (int64_t)k + 4] != 0.0 ? 1 : 0;
  nu = block_sum_int(nu, red, t);
  if (nu < EP_MIN_MATCHES) return pair_fails(a, pr, k0, k1, t, BA_RP_FEW_MATCHES, 0, -1);
  if (!pair_focals_ok(in)) return pair_fails(a, pr, k0, k1, t, BA_RP_DEGENERATE, 0, -1);
  if (a.hypotheses == 0) {
    for (int k = k0 + t; k < k1; k += PR_BLK) a.inlier[k] = a.rays[PAIR_RAY * (int64_t)k + 4] != 0.0 ? 1 : 0;
    if (t == 0) a.status[pr] = BA_RP_OK, a.n_inliers[pr] = nu, a.best_hyp[pr] = -1, a.stopped[pr] = 0;
    return;
  }
  int best, best_count;
  consensus_winner(a.hyp_count + (int64_t)pr * a.hypotheses, a.hypotheses, t, redk, best, best_count);
  if (best < 0 || best_count < a.min_inliers) return pair_fails(a, pr, k0, k1, t, BA_RP_NO_CONSENSUS, best_count, best);
  const double *win = a.hyp_pose + PAIR_HYP_DOUBLES * ((int64_t)pr * a.hypotheses + best);
  PairPose P;
  pair_pose_of(win, win + 3, P);
  const int n = consensus_mark(
      k0, k1, a.inlier, red, t, [](int k) { return k; },
      [&](int k) { return pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2); });
  if (t == 0) a.status[pr] = BA_RP_OK, a.n_inliers[pr] = n, a.best_hyp[pr] = best, a.stopped[pr] = 0;
}

// the LDS of k_pair_fit: the fit's scratch, the four waves' partial sums, the first match of the set
struct PairFitShared {
  PairScratch ps;
  double part[PR_WAVES][EP_SUMS];
  double st[6];
  int red[PR_WAVES];
};

// part[wave][i] <- the wave's sum of v (every lane passes its partial sum); the caller puts a barrier behind the last of them
__device__ __forceinline__ void pair_wave_part(PairFitShared &sh, int i, double v, int t) {
  v = wave_all_sum(v);
  if ((t & 63) == 0) sh.part[t >> 6][i] = v;
}

// the LDS of k_pair_refine
struct PairRefineShared {
  PairFitShared fit;           // the waves' partial sums, the integer sums, and (ps.rs) the scratch of rotation_vector
  double S[RP_SUMS];           // F, g, H at the current pose
  double R[9], t[3], E[9];     // the current pose
  double B[6], G[9 * RP_DOF];  // its tangent basis and the five dE
  double Rn[9], tn[3], En[9];  // the trial pose
  double delta[RP_DOF], L[RP_HESS], W[9], ret[6];
  double Fn;
  int ok;
};

// out[i] <- the sum of acc[i] over the workgroup in the fixed order of k_pair_fit, i < N; a barrier behind it
template <int N>
__device__ __forceinline__ void pair_refine_reduce(PairRefineShared &sh, const double (&acc)[N], double *out, int t) {
#pragma unroll
  for (int i = 0; i < N; i++) pair_wave_part(sh.fit, i, acc[i], t);
  __syncthreads();
  if (t < N) out[t] = ((sh.fit.part[0][t] + sh.fit.part[1][t]) + sh.fit.part[2][t]) + sh.fit.part[3][t];
  __syncthreads();
}

// sh.S <- F = 1/2 sum c^2 rho(e^2 / c^2), g = sum w J'e, H = sum w J'J over the set at the current pose (sh.E, sh.G), w = rho'
__device__ __forceinline__ void pair_refine_sums(const PairArgs &a, const PairRefineArgs &q, PairRefineShared &sh, int k0, int k1, double fa,
                                                 double fb, int t) {
  double acc[RP_SUMS];
#pragma unroll
  for (int i = 0; i < RP_SUMS; i++) acc[i] = 0.0;
  for (int k = k0 + t; k < k1; k += PR_BLK)
    if (a.inlier[k] & 1) {
      const double *ray = a.rays + PAIR_RAY * (int64_t)k;
      double l[2], m[2], n, D, J[RP_DOF], w;
      const double e = pair_sampson_signed(ray, sh.E, fa, fb, l, m, n, D);
      pair_sampson_jacobian(ray, sh.G, fa, fb, l, m, n, D, J);
      acc[0] += 0.5 * robust_rho(q.loss, e * e, q.c2, &w);
      int tt = 1 + RP_DOF;
#pragma unroll
      for (int i = 0; i < RP_DOF; i++) {
        const double wj = w * J[i];
        acc[1 + i] += wj * e;
#pragma unroll
        for (int j = 0; j <= i; j++, tt++) acc[tt] += wj * J[j];
      }
    }
  pair_refine_reduce<RP_SUMS>(sh, acc, sh.S, t);
}

// sh.Fn <- F over the set at the trial pose (sh.En)
__device__ __forceinline__ void pair_refine_cost(const PairArgs &a, const PairRefineArgs &q, PairRefineShared &sh, int k0, int k1, double fa,
                                                 double fb, int t) {
  double acc[1] = {0.0};
  for (int k = k0 + t; k < k1; k += PR_BLK)
    if (a.inlier[k] & 1) {
      double l[2], m[2], n, D, w;
      const double e = pair_sampson_signed(a.rays + PAIR_RAY * (int64_t)k, sh.En, fa, fb, l, m, n, D);
      acc[0] += 0.5 * robust_rho(q.loss, e * e, q.c2, &w);
    }
  pair_refine_reduce<1>(sh, acc, &sh.Fn, t);
}

// One pair per workgroup (ba_refine_relative_pose): the Marquardt iteration of the header on the pair's current set M
// (the inlier bytes) from its current pose (a.pose), the whole loop in this launch; then |M'|, the set of the whole list under
// the refined pose.  round 0 first takes the caller's set down to its used members and decides SKIPPED.  final == 0: M' goes
// through the adopt rule of consensus_rescore; the pair stops when it is not adopted.  Every decision is taken on values all
// threads share: they come out of LDS behind a barrier.
__global__ __launch_bounds__(PR_BLK) void k_pair_refine(PairArgs a, PairRefineArgs q, int round, int final) {
  __shared__ PairRefineShared sh;
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  double *pose = a.pose + 6 * (int64_t)pr;
  int n_set;
  if (round == 0) {
    int n = 0;
    for (int k = k0 + t; k < k1; k += PR_BLK) {
      const int member = ((q.all_used || (a.inlier[k] & 1)) && a.rays[PAIR_RAY * (int64_t)k + 4] != 0.0) ? 1 : 0;
      a.inlier[k] = (uint8_t)member;
      n += member;
    }
    n_set = block_sum_int(n, sh.fit.red, t);
    const bool skip = a.status[pr] != BA_RP_OK || !pair_focals_ok(in) || n_set < RP_MIN_SET;
    if (t == 0) {
      a.stopped[pr] = skip ? 1 : 0, a.n_inliers[pr] = n_set;
      q.state[pr] = BA_RR_SKIPPED, q.iters[pr] = 0, q.n_consistent[pr] = 0;
      q.cost[2 * (int64_t)pr] = 0.0, q.cost[2 * (int64_t)pr + 1] = 0.0;
    }
    if (skip) return;
  } else {
    if (a.stopped[pr]) return;
    n_set = a.n_inliers[pr];
  }
  const double fa = in[2], fb = in[5];
  if (t == 0) {
    PairPose P;
    pair_pose_of(pose, pose + 3, P);
#pragma unroll
    for (int e = 0; e < 9; e++) sh.R[e] = P.R[e], sh.E[e] = P.E[e];
#pragma unroll
    for (int e = 0; e < 3; e++) sh.t[e] = P.t[e];
    pair_tangent(sh.R, sh.t, sh.B, sh.G, sh.W);
  }
  __syncthreads();
  pair_refine_sums(a, q, sh, k0, k1, fa, fb, t);
  double F = sh.S[0];
  if (round == 0 && t == 0) q.cost[2 * (int64_t)pr] = F;
  if (!isfinite(F)) {
    if (t == 0) q.state[pr] = BA_RR_NONFINITE, q.cost[2 * (int64_t)pr + 1] = F, a.stopped[pr] = 1;
    return;
  }
  int state = BA_RR_MAX_ITER, trials = 0;
  bool fresh = true, moved = false;  // fresh: sh.S holds the sums of the current pose
  double lam = q.lambda0;
#pragma nounroll
  for (int it = 0; it < q.max_iter; it++) {
    trials = it + 1;
    __syncthreads();  // (every thread has read the last trial's ok, Fn and delta)
    if (!fresh) pair_refine_sums(a, q, sh, k0, k1, fa, fb, t);
    fresh = true;
    if (t == 0) {
      const bool ok = pair_step(sh.S, lam, sh.L, sh.delta);
      if (ok) pair_retract(sh.R, sh.t, sh.B, sh.delta, sh.Rn, sh.tn, sh.En, sh.W);
      sh.ok = ok ? 1 : 0;
    }
    __syncthreads();
    bool accept = false;
    if (sh.ok) {
      pair_refine_cost(a, q, sh, k0, k1, fa, fb, t);
      accept = isfinite(sh.Fn) && sh.Fn <= F;
    }
    if (accept) {
      F = sh.Fn;
      if (t == 0) {
        for (int e = 0; e < 9; e++) sh.R[e] = sh.Rn[e], sh.E[e] = sh.En[e];
        for (int e = 0; e < 3; e++) sh.t[e] = sh.tn[e];
        pair_tangent(sh.R, sh.t, sh.B, sh.G, sh.W);
      }
      fresh = false, moved = true;
      lam = fmax(lam / 10.0, 1e-12);
      double nd = 0.0;
#pragma unroll
      for (int i = 0; i < RP_DOF; i++) nd += sh.delta[i] * sh.delta[i];
      if (sqrt(nd) <= q.xtol) {
        state = BA_RR_CONVERGED;
        break;
      }
    } else {
      lam *= 10.0;
      if (lam > 1e12) {
        state = BA_RR_STALLED;
        break;
      }
    }
  }
  if (t == 0) {
    if (moved) {  // (a pose that no step moved keeps its bits)
      for (int e = 0; e < 9; e++) sh.fit.ps.rs.R[e] = sh.R[e];
      rotation_vector(sh.fit.ps.rs);
      for (int e = 0; e < 3; e++) pose[e] = sh.fit.ps.rs.r[e], pose[3 + e] = sh.t[e];
    }
    for (int e = 0; e < 6; e++) sh.ret[e] = pose[e];
    q.state[pr] = (uint8_t)state, q.cost[2 * (int64_t)pr + 1] = F, q.iters[pr] += trials;
  }
  __syncthreads();
  PairPose P;
  pair_pose_of(sh.ret, sh.ret + 3, P);
  int nc = 0;
  for (int k = k0 + t; k < k1; k += PR_BLK) nc += pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, fa, fb, a.tau2) ? 1 : 0;
  nc = block_sum_int(nc, sh.fit.red, t);
  if (t == 0) q.n_consistent[pr] = nc;
  if (final) return;
  const int n = consensus_rescore(
      k0, k1, n_set, a.inlier, sh.fit.red, t, [](int k) { return k; },
      [&](int k) { return pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, fa, fb, a.tau2); });
  if (t == 0) {
    if (n >= 0) a.n_inliers[pr] = n;
    else a.stopped[pr] = 1;
  }
}

// One pair per workgroup: the linear fit on its current set M (the inlier bytes).  final == 0, a round of the refits: the adopt
// rule of consensus_rescore on the whole list under the fit; M stays and the pair stops when M' is not adopted, and when the fit
// is degenerate.  final != 0: the pose of the fit -> a.pose, or the state DEGENERATE.
__global__ __launch_bounds__(PR_BLK) void k_pair_fit(PairArgs a, int final) {
  __shared__ PairFitShared sh;
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  if (a.status[pr] != BA_RP_OK || (!final && a.stopped[pr])) return;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  const int n_old = a.n_inliers[pr];
  PairScratch &ps = sh.ps;
  // the first match of the set: the provisional origin
  int first = k1;
  for (int k = k0 + t; k < k1; k += PR_BLK)
    if ((a.inlier[k] & 1) && k < first) first = k;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int other = __shfl_xor(first, off, 64);
    first = other < first ? other : first;
  }
  if ((t & 63) == 0) sh.red[t >> 6] = first;
  __syncthreads();
  for (int w = 0; w < PR_WAVES; w++) first = sh.red[w] < first ? sh.red[w] : first;
  bool ok = first < k1;  // (every decision below is taken on values all threads share)
  double oa[2] = {0.0, 0.0}, ob[2] = {0.0, 0.0}, dma[3], dmb[3], sa = 0.0, sb = 0.0;
  if (ok) {
    const double *r0 = a.rays + PAIR_RAY * (int64_t)first;
    oa[0] = r0[0], oa[1] = r0[1], ob[0] = r0[2], ob[1] = r0[3];
    double mo[6] = {0, 0, 0, 0, 0, 0};
    for (int k = k0 + t; k < k1; k += PR_BLK)
      if (a.inlier[k] & 1) {
        const double *ray = a.rays + PAIR_RAY * (int64_t)k;
        const double ax = ray[0] - oa[0], ay = ray[1] - oa[1], bx = ray[2] - ob[0], by = ray[3] - ob[1];
        mo[0] += ax, mo[1] += ay, mo[2] += ax * ax + ay * ay;
        mo[3] += bx, mo[4] += by, mo[5] += bx * bx + by * by;
      }
#pragma unroll
    for (int i = 0; i < 6; i++) pair_wave_part(sh, i, mo[i], t);
    __syncthreads();
    if (t < 6) sh.st[t] = ((sh.part[0][t] + sh.part[1][t]) + sh.part[2][t]) + sh.part[3][t];
    __syncthreads();
    ok = image_stats((double)n_old, sh.st[0], sh.st[1], sh.st[2], dma, sa) && image_stats((double)n_old, sh.st[3], sh.st[4], sh.st[5], dmb, sb);
  }
  if (ok) {
    double acc[EP_SUMS];
#pragma unroll
    for (int i = 0; i < EP_SUMS; i++) acc[i] = 0.0;
    for (int k = k0 + t; k < k1; k += PR_BLK)
      if (a.inlier[k] & 1) {
        const double *ray = a.rays + PAIR_RAY * (int64_t)k;
        double da[3], db[3], term[EP_SUMS];
        normalised_ray(ray[0], ray[1], oa, dma, sa, da);
        normalised_ray(ray[2], ray[3], ob, dmb, sb, db);
        epipolar_terms(da, db, term);
#pragma unroll
        for (int i = 0; i < EP_SUMS; i++) acc[i] += term[i];
      }
#pragma unroll
    for (int i = 0; i < EP_SUMS; i++) pair_wave_part(sh, i, acc[i], t);
    __syncthreads();
    if (t < EP_SUMS) ps.S[t] = ((sh.part[0][t] + sh.part[1][t]) + sh.part[2][t]) + sh.part[3][t];
    __syncthreads();
    for (int i = 0; i < EP_SUMS; i++) ok = ok && isfinite(ps.S[i]);
  }
  if (ok) {
    const double ca[2] = {oa[0] + dma[0], oa[1] + dma[1]}, cb[2] = {ob[0] + dmb[0], ob[1] + dmb[1]};
    ok = essential_from_sums<__syncthreads>(ps, t, PR_BLK, ca, sa, cb, sb);
  }
  if (ok) {  // the matches of the set in front of both cameras, per candidate
    int cnt[4] = {0, 0, 0, 0};
    for (int k = k0 + t; k < k1; k += PR_BLK)
      if (a.inlier[k] & 1) {
        const double *ray = a.rays + PAIR_RAY * (int64_t)k;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          double al, be;
          pair_depths(ps.Rc + 9 * (c >> 1), ps.tn, (c & 1) ? -1.0 : 1.0, ray[0], ray[1], ray[2], ray[3], al, be);
          cnt[c] += (al > 0.0 && be > 0.0) ? 1 : 0;
        }
      }
#pragma unroll
    for (int c = 0; c < 4; c++) cnt[c] = block_sum_int(cnt[c], sh.red, t);
    if (t == 0) {
#pragma unroll
      for (int c = 0; c < 4; c++) ps.cnt[c] = cnt[c];
      ps.ok = pair_pose_winner(ps) ? 1 : 0;
    }
    __syncthreads();
    ok = ps.ok != 0;
  }
  if (final) {
    if (t == 0 && !ok) a.status[pr] = BA_RP_DEGENERATE;
    if (ok && t < 3) a.pose[6 * (int64_t)pr + t] = ps.rs.r[t], a.pose[6 * (int64_t)pr + 3 + t] = ps.t[t];
    return;
  }
  if (!ok) {
    if (t == 0) a.stopped[pr] = 1;
    return;
  }
  PairPose P;
  pair_pose_of(ps.rs.r, ps.t, P);
  const int n = consensus_rescore(
      k0, k1, n_old, a.inlier, sh.red, t, [](int k) { return k; },
      [&](int k) { return pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2); });
  if (t == 0) {
    if (n >= 0) a.n_inliers[pr] = n;
    else a.stopped[pr] = 1;
  }
}

// The match lists of the pairs (a, b) (1-based) over the observation lists cam / pnt (indices with the given base): the walk of
// the header.  ptr: npairs + 1 offsets; oa, ob (either both or neither): the 0-based observations of every match.
// BA_ERR_ARG (message with `who`): a pair with a == b or an index outside 1..ncams, an observation index out of range.
template <typename I>
int pair_match_lists(const char *who, int64_t ncams, int64_t npnts, int64_t nobs, const I *cam, const I *pnt, int64_t base, int64_t npairs,
                     const int64_t *pair_a1, const int64_t *pair_b1, std::vector<int64_t> &ptr, std::vector<int64_t> *oa, std::vector<int64_t> *ob) {
  for (int64_t k = 0; k < nobs; k++) {
    const int64_t c = (int64_t)cam[k] - base, q = (int64_t)pnt[k] - base;
    if (c < 0 || c >= ncams || q < 0 || q >= npnts) {
      ba_set_error("%s: observation %lld has a camera or point index out of range", who, (long long)k + 1);
      return BA_ERR_ARG;
    }
  }
  for (int64_t i = 0; i < npairs; i++)
    if (pair_a1[i] < 1 || pair_a1[i] > ncams || pair_b1[i] < 1 || pair_b1[i] > ncams || pair_a1[i] == pair_b1[i]) {
      ba_set_error("%s: pair %lld is (%lld, %lld): two different cameras in 1..%lld", who, (long long)i + 1, (long long)pair_a1[i],
                   (long long)pair_b1[i], (long long)ncams);
      return BA_ERR_ARG;
    }
  // every camera's observations in the caller's order
  std::vector<int64_t> cptr((size_t)ncams + 1, 0), cobs((size_t)nobs);
  for (int64_t k = 0; k < nobs; k++) cptr[(size_t)((int64_t)cam[k] - base) + 1]++;
  for (int64_t c = 0; c < ncams; c++) cptr[(size_t)c + 1] += cptr[(size_t)c];
  {
    std::vector<int64_t> at(cptr.begin(), cptr.end() - 1);
    for (int64_t k = 0; k < nobs; k++) cobs[(size_t)at[(size_t)((int64_t)cam[k] - base)]++] = k;
  }
  // seen_a[P] / seen_b[P] == i + 1: pair i has met point P in that camera's list; first_b[P]: b's first observation of it
  std::vector<int64_t> seen_a((size_t)npnts, 0), seen_b((size_t)npnts, 0), first_b((size_t)npnts, 0);
  ptr.assign((size_t)npairs + 1, 0);
  for (int64_t i = 0; i < npairs; i++) {
    const int64_t ca = pair_a1[i] - 1, cb = pair_b1[i] - 1;
    for (int64_t j = cptr[(size_t)cb]; j < cptr[(size_t)cb + 1]; j++) {
      const int64_t o = cobs[(size_t)j], q = (int64_t)pnt[o] - base;
      if (seen_b[(size_t)q] != i + 1) seen_b[(size_t)q] = i + 1, first_b[(size_t)q] = o;
    }
    int64_t n = 0;
    for (int64_t j = cptr[(size_t)ca]; j < cptr[(size_t)ca + 1]; j++) {
      const int64_t o = cobs[(size_t)j], q = (int64_t)pnt[o] - base;
      if (seen_a[(size_t)q] == i + 1) continue;
      seen_a[(size_t)q] = i + 1;
      if (seen_b[(size_t)q] != i + 1) continue;
      n++;
      if (oa) oa->push_back(o), ob->push_back(first_b[(size_t)q]);
    }
    ptr[(size_t)i + 1] = ptr[(size_t)i] + n;
  }
  return BA_OK;
}

// d <- h (n elements, d holds at least n) on st; the host vector outlives the call's synchronisation
template <typename T>
int pair_upload(T *d, const std::vector<T> &h, hipStream_t st) {
  if (!h.empty()) BA_HIP_CHECK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return BA_OK;
}

// the buffers of a call with npairs pairs, nmatch matches and H hypotheses per pair: grown, never shrunk
int pair_buffers(PairWork &w, int64_t npairs, int64_t nmatch, int64_t H) {
  if (w.pair_cap < npairs) {
    w.pair_cap = 0;
    BA_CHECK(w.match_ptr.alloc(npairs + 1));
    BA_CHECK(w.intr.alloc(6 * npairs));
    BA_CHECK(w.pose.alloc(6 * npairs));
    BA_CHECK(w.n_inliers.alloc(npairs));
    BA_CHECK(w.best_hyp.alloc(npairs));
    BA_CHECK(w.stopped.alloc(npairs));
    BA_CHECK(w.status.alloc(npairs));
    w.pair_cap = npairs;
    w.hyp_cap = 0;  // (the hypothesis records are per pair)
  }
  if (w.match_cap < nmatch || !w.rays) {
    w.match_cap = 0;
    BA_CHECK(w.obs_a.alloc(nmatch));
    BA_CHECK(w.obs_b.alloc(nmatch));
    BA_CHECK(w.pair_of.alloc(nmatch));
    BA_CHECK(w.rays.alloc(PAIR_RAY * nmatch));
    BA_CHECK(w.inlier.alloc(nmatch));
    w.match_cap = nmatch;
  }
  if (w.hyp_cap < w.pair_cap * H) {
    w.hyp_cap = 0;
    BA_CHECK(w.hyp_pose.alloc(PAIR_HYP_DOUBLES * w.pair_cap * H));
    BA_CHECK(w.hyp_count.alloc(w.pair_cap * H));
    w.hyp_cap = w.pair_cap * H;
  }
  return BA_OK;
}

// the host copies of what a call uploads: they outlive the call's synchronisation
struct PairUpload {
  std::vector<int> ptr, oa, ob, pair;
  std::vector<double> intr;
};

// What every entry with match lists does first on the device: the lists (ptr, oa, ob of pair_match_lists) as int32 and the six
// intrinsics of every pair uploaded into the buffers (grown for H hypotheses per pair), the handle's information array, the
// pointers of `a`, and the ray records (k_pair_rays).  npairs > 0.
int pair_front(ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const std::vector<int64_t> &ptr,
               const std::vector<int64_t> &oa, const std::vector<int64_t> &ob, int64_t H, PairUpload &h, PairArgs &a) {
  const int64_t nmatch = ptr[(size_t)npairs];
  h.ptr.assign(ptr.begin(), ptr.end()), h.oa.assign(oa.begin(), oa.end()), h.ob.assign(ob.begin(), ob.end());
  h.pair.resize((size_t)nmatch), h.intr.resize((size_t)(6 * npairs));
  for (int64_t i = 0; i < npairs; i++) {
    for (int64_t k = ptr[(size_t)i]; k < ptr[(size_t)i + 1]; k++) h.pair[(size_t)k] = (int)i;
    const double *ca = x + 3 * p->npnts + 9 * (pair_a1[i] - 1), *cb = x + 3 * p->npnts + 9 * (pair_b1[i] - 1);
    for (int j = 0; j < 3; j++) h.intr[(size_t)(6 * i + j)] = ca[6 + j], h.intr[(size_t)(6 * i + 3 + j)] = cb[6 + j];
  }
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  BA_CHECK(info_upload(p));
  PairWork &w = p->pairs;
  BA_CHECK(pair_buffers(w, npairs, nmatch, H));
  BA_CHECK(pair_upload((int *)w.match_ptr, h.ptr, st));
  BA_CHECK(pair_upload((int *)w.obs_a, h.oa, st));
  BA_CHECK(pair_upload((int *)w.obs_b, h.ob, st));
  BA_CHECK(pair_upload((int *)w.pair_of, h.pair, st));
  BA_CHECK(pair_upload((double *)w.intr, h.intr, st));
  a.match_ptr = w.match_ptr, a.obs_a = w.obs_a, a.obs_b = w.obs_b, a.pair_of = w.pair_of;
  a.intr = w.intr, a.pt2d = p->pt2d, a.info = p->info_on() ? (const double *)p->d_info : nullptr;
  a.rays = w.rays, a.hyp_pose = w.hyp_pose, a.pose = w.pose;
  a.hyp_count = w.hyp_count, a.n_inliers = w.n_inliers, a.best_hyp = w.best_hyp;
  a.inlier = w.inlier, a.stopped = w.stopped, a.status = w.status;
  return BA_LAUNCH(k_pair_rays, grid_for(nmatch, PR_BLK), PR_BLK, 0, st, a, nmatch);
}

}  // namespace

extern "C" int ba_pair_matches(int64_t ncams, int64_t npnts, int64_t nobs, const int64_t *cam_idx1, const int64_t *pnt_idx1, int64_t npairs,
                               const int64_t *pair_a1, const int64_t *pair_b1, int64_t *match_ptr, int64_t *obs_a1, int64_t *obs_b1) {
  if (ncams < 0 || npnts < 0 || nobs < 0 || npairs < 0 || (nobs > 0 && (!cam_idx1 || !pnt_idx1)) || (npairs > 0 && (!pair_a1 || !pair_b1)) ||
      !match_ptr || (obs_a1 == nullptr) != (obs_b1 == nullptr)) {
    ba_set_error("ba_pair_matches: null argument or negative size (obs_a1 and obs_b1: both or neither)");
    return BA_ERR_ARG;
  }
  std::vector<int64_t> ptr, oa, ob;
  BA_CHECK(pair_match_lists("ba_pair_matches", ncams, npnts, nobs, cam_idx1, pnt_idx1, 1, npairs, pair_a1, pair_b1, ptr, obs_a1 ? &oa : nullptr,
                            obs_a1 ? &ob : nullptr));
  for (size_t i = 0; i < ptr.size(); i++) match_ptr[i] = ptr[i];
  for (size_t k = 0; k < oa.size(); k++) obs_a1[k] = oa[k] + 1, obs_b1[k] = ob[k] + 1;
  return BA_OK;
}

namespace {

// ba_relative_pose (five == false) and ba_relative_pose_five_point (five == true): one host path, the hypothesis kernel differs
int relative_pose_call(const char *who, bool five, ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1,
                       const int64_t *pair_b1, const ba_ransac_opts *opts, double *pose, uint8_t *status, int64_t *match_ptr,
                       uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp, int64_t *counts) {
  ba_ransac_opts o = {};
  if (five) BA_CHECK(ransac_opts_check(who, opts, &o, FP_POINTS, EP_MIN_MATCHES, FP_POINTS));
  else if (opts) BA_CHECK(ransac_opts_check(who, opts, &o, EP_MIN_MATCHES));
  if (!p || npairs < 0 || (npairs > 0 && (!x || !pair_a1 || !pair_b1 || !pose || !status))) {
    ba_set_error("%s: null argument or npairs < 0", who);
    return BA_ERR_ARG;
  }
  if (p->comm.active()) {
    ba_set_error("%s: not supported on a handle with a communicator (a camera's observations are spread over the shards)", who);
    return BA_ERR_ARG;
  }
  std::vector<int64_t> ptr, oa, ob;
  BA_CHECK(pair_match_lists(who, p->ncams, p->npnts, p->nobs, p->h_cam0.data(), p->h_pnt0.data(), 0, npairs, pair_a1, pair_b1, ptr, &oa, &ob));
  const int64_t nmatch = ptr[(size_t)npairs];
  if (nmatch > (int64_t)INT32_MAX) {
    ba_set_error("%s: %lld matches: more than 2^31 - 1", who, (long long)nmatch);
    return BA_ERR_ARG;
  }
  if (match_ptr)
    for (size_t i = 0; i < ptr.size(); i++) match_ptr[i] = ptr[i];
  if (counts)
    for (int s = 0; s < BA_RP_STATES; s++) counts[s] = 0;
  if (npairs == 0) return BA_OK;
  hipStream_t st = p->stream;
  PairWork &w = p->pairs;
  PairUpload up;
  PairArgs a = {};
  BA_CHECK(pair_front(p, x, npairs, pair_a1, pair_b1, ptr, oa, ob, opts ? o.hypotheses : 0, up, a));
  a.hypotheses = opts ? o.hypotheses : 0, a.sample = o.sample, a.min_inliers = o.min_inliers;
  a.seed_mix = ransac_seed_mix(o.seed), a.tau2 = o.threshold * o.threshold;
  if (five) BA_CHECK(BA_LAUNCH(k_pair_hypotheses5, dim3((unsigned)npairs, grid_for(o.hypotheses, PR_WAVES)), PR_BLK, 0, st, a));
  else if (opts) BA_CHECK(BA_LAUNCH(k_pair_hypotheses, dim3((unsigned)npairs, grid_for(o.hypotheses, PR_WAVES)), PR_BLK, 0, st, a));
  BA_CHECK(BA_LAUNCH(k_pair_select, (unsigned)npairs, PR_BLK, 0, st, a));
  for (int it = 0; opts && it < o.refits; it++) BA_CHECK(BA_LAUNCH(k_pair_fit, (unsigned)npairs, PR_BLK, 0, st, a, 0));
  BA_CHECK(BA_LAUNCH(k_pair_fit, (unsigned)npairs, PR_BLK, 0, st, a, 1));
  std::vector<double> h_pose((size_t)(6 * npairs));
  std::vector<uint8_t> h_status((size_t)npairs);
  BA_HIP_CHECK(hipMemcpyAsync(h_pose.data(), w.pose, h_pose.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_status.data(), w.status, h_status.size(), hipMemcpyDeviceToHost, st));
  if (inlier && nmatch > 0) BA_HIP_CHECK(hipMemcpyAsync(inlier, w.inlier, (size_t)nmatch, hipMemcpyDeviceToHost, st));
  if (n_inliers) BA_HIP_CHECK(hipMemcpyAsync(n_inliers, w.n_inliers, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (best_hyp) BA_HIP_CHECK(hipMemcpyAsync(best_hyp, w.best_hyp, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < npairs; i++) {
    const uint8_t s = h_status[(size_t)i];
    status[i] = s;
    if (counts && s < BA_RP_STATES) counts[s]++;
    if (s == BA_RP_OK)  // (a pair in any other state leaves its six entries as the caller filled them)
      for (int j = 0; j < 6; j++) pose[6 * i + j] = h_pose[(size_t)(6 * i + j)];
  }
  return BA_OK;
}

}  // namespace

extern "C" int ba_relative_pose(ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                                const ba_ransac_opts *opts, double *pose, uint8_t *status, int64_t *match_ptr, uint8_t *inlier,
                                int32_t *n_inliers, int32_t *best_hyp, int64_t *counts) {
  return relative_pose_call("ba_relative_pose", false, p, x, npairs, pair_a1, pair_b1, opts, pose, status, match_ptr, inlier, n_inliers,
                            best_hyp, counts);
}

extern "C" int ba_relative_pose_five_point(ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                                           const ba_ransac_opts *opts, double *pose, uint8_t *status, int64_t *match_ptr,
                                           uint8_t *inlier, int32_t *n_inliers, int32_t *best_hyp, int64_t *counts) {
  return relative_pose_call("ba_relative_pose_five_point", true, p, x, npairs, pair_a1, pair_b1, opts, pose, status, match_ptr, inlier,
                            n_inliers, best_hyp, counts);
}

extern "C" int ba_five_point(ba_problem *p, int64_t n, const double *qa, const double *qb, double *E, int32_t *n_sol) {
  if (!p || n < 0 || (n > 0 && (!qa || !qb || !E || !n_sol))) {
    ba_set_error("ba_five_point: null argument or n < 0");
    return BA_ERR_ARG;
  }
  if (n > (int64_t)INT32_MAX / (9 * FP_MAX_SOL)) {
    ba_set_error("ba_five_point: %lld tuples: more than %lld", (long long)n, (long long)(INT32_MAX / (9 * FP_MAX_SOL)));
    return BA_ERR_ARG;
  }
  if (n == 0) return BA_OK;
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  PairWork &w = p->pairs;
  if (w.five_cap < n) {
    w.five_cap = 0;
    BA_CHECK(w.five_qa.alloc(2 * FP_POINTS * n));
    BA_CHECK(w.five_qb.alloc(2 * FP_POINTS * n));
    BA_CHECK(w.five_E.alloc(9 * FP_MAX_SOL * n));
    BA_CHECK(w.five_n.alloc(n));
    w.five_cap = n;
  }
  const size_t in_bytes = (size_t)(2 * FP_POINTS * n) * sizeof(double);
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.five_qa, qa, in_bytes, hipMemcpyHostToDevice, st));
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.five_qb, qb, in_bytes, hipMemcpyHostToDevice, st));
  BA_CHECK(BA_LAUNCH(k_five_point, grid_for(n, PR_WAVES), PR_BLK, 0, st, n, w.five_qa, w.five_qb, w.five_E, w.five_n));
  BA_HIP_CHECK(hipMemcpyAsync(E, w.five_E, (size_t)(9 * FP_MAX_SOL * n) * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(n_sol, w.five_n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

int pair_refine_opts_check(const char *who, const ba_pair_refine_opts *in, ba_pair_refine_opts *o) {
  if (!in) {
    ba_set_error("%s: null options", who);
    return BA_ERR_ARG;
  }
  *o = *in;
  if (!std::isfinite(o->xtol) || !std::isfinite(o->lambda0)) {
    ba_set_error("%s: xtol and lambda0 must be finite (<= 0: %g and %g), got %g, %g", who, RR_XTOL_DEFAULT, RR_LAMBDA0_DEFAULT, o->xtol,
                 o->lambda0);
    return BA_ERR_ARG;
  }
  if (o->loss < BA_LOSS_LINEAR || o->loss > BA_LOSS_ARCTAN || !std::isfinite(o->f_scale) || !(o->f_scale > 0)) {
    ba_set_error("%s: loss must be one of BA_LOSS_* and f_scale finite and > 0 (pixels), got %d, %g", who, o->loss, o->f_scale);
    return BA_ERR_ARG;
  }
  if (!std::isfinite(o->threshold) || !(o->threshold > 0)) {
    ba_set_error("%s: threshold must be finite and > 0 (pixels), got %g", who, o->threshold);
    return BA_ERR_ARG;
  }
  if (o->max_iter < 0) o->max_iter = RR_MAX_ITER_DEFAULT;
  if (o->xtol <= 0) o->xtol = RR_XTOL_DEFAULT;
  if (o->lambda0 <= 0) o->lambda0 = RR_LAMBDA0_DEFAULT;
  if (o->rounds < 0) o->rounds = RR_ROUNDS_DEFAULT;
  if (o->rounds > RR_ROUNDS_MAX) {
    ba_set_error("%s: rounds must be <= %d, got %d", who, RR_ROUNDS_MAX, o->rounds);
    return BA_ERR_ARG;
  }
  return BA_OK;
}

extern "C" int ba_refine_relative_pose(ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                                       const ba_pair_refine_opts *opts, double *pose_inout, const uint8_t *status_in, uint8_t *inlier_inout,
                                       uint8_t *state, double *cost, int32_t *n_inliers, int32_t *n_consistent, int32_t *iters,
                                       int64_t *counts) {
  const char *who = "ba_refine_relative_pose";
  ba_pair_refine_opts o = {};
  BA_CHECK(pair_refine_opts_check(who, opts, &o));
  if (!p || npairs < 0 || (npairs > 0 && (!x || !pair_a1 || !pair_b1 || !pose_inout || !state))) {
    ba_set_error("%s: null argument or npairs < 0", who);
    return BA_ERR_ARG;
  }
  if (p->comm.active()) {
    ba_set_error("%s: not supported on a handle with a communicator (a camera's observations are spread over the shards)", who);
    return BA_ERR_ARG;
  }
  std::vector<int64_t> ptr, oa, ob;
  BA_CHECK(pair_match_lists(who, p->ncams, p->npnts, p->nobs, p->h_cam0.data(), p->h_pnt0.data(), 0, npairs, pair_a1, pair_b1, ptr, &oa, &ob));
  const int64_t nmatch = ptr[(size_t)npairs];
  if (nmatch > (int64_t)INT32_MAX) {
    ba_set_error("%s: %lld matches: more than 2^31 - 1", who, (long long)nmatch);
    return BA_ERR_ARG;
  }
  if (counts)
    for (int s = 0; s < BA_RR_STATES; s++) counts[s] = 0;
  if (npairs == 0) return BA_OK;
  hipStream_t st = p->stream;
  PairWork &w = p->pairs;
  PairUpload up;
  PairArgs a = {};
  BA_CHECK(pair_front(p, x, npairs, pair_a1, pair_b1, ptr, oa, ob, 0, up, a));
  if (w.rr_cap < npairs) {
    w.rr_cap = 0;
    BA_CHECK(w.rr_state.alloc(npairs));
    BA_CHECK(w.rr_cost.alloc(2 * npairs));
    BA_CHECK(w.rr_consistent.alloc(npairs));
    BA_CHECK(w.rr_iters.alloc(npairs));
    w.rr_cap = npairs;
  }
  a.tau2 = o.threshold * o.threshold;
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.pose, pose_inout, (size_t)(6 * npairs) * sizeof(double), hipMemcpyHostToDevice, st));
  if (status_in) BA_HIP_CHECK(hipMemcpyAsync((uint8_t *)w.status, status_in, (size_t)npairs, hipMemcpyHostToDevice, st));
  else BA_HIP_CHECK(hipMemsetAsync((uint8_t *)w.status, BA_RP_OK, (size_t)npairs, st));
  if (inlier_inout && nmatch > 0) BA_HIP_CHECK(hipMemcpyAsync((uint8_t *)w.inlier, inlier_inout, (size_t)nmatch, hipMemcpyHostToDevice, st));
  PairRefineArgs q;
  q.state = w.rr_state, q.cost = w.rr_cost, q.n_consistent = w.rr_consistent, q.iters = w.rr_iters;
  q.max_iter = o.max_iter, q.loss = o.loss, q.all_used = inlier_inout ? 0 : 1;
  q.xtol = o.xtol, q.lambda0 = o.lambda0, q.c2 = o.f_scale * o.f_scale;
  for (int round = 0; round <= o.rounds; round++)
    BA_CHECK(BA_LAUNCH(k_pair_refine, (unsigned)npairs, PR_BLK, 0, st, a, q, round, round == o.rounds ? 1 : 0));
  std::vector<double> h_pose((size_t)(6 * npairs)), h_cost((size_t)(2 * npairs));
  std::vector<uint8_t> h_state((size_t)npairs), h_inlier((size_t)nmatch);
  std::vector<int32_t> h_n((size_t)npairs), h_nc((size_t)npairs), h_it((size_t)npairs);
  BA_HIP_CHECK(hipMemcpyAsync(h_pose.data(), w.pose, h_pose.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_cost.data(), w.rr_cost, h_cost.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_state.data(), w.rr_state, h_state.size(), hipMemcpyDeviceToHost, st));
  if (inlier_inout && nmatch > 0) BA_HIP_CHECK(hipMemcpyAsync(h_inlier.data(), w.inlier, (size_t)nmatch, hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_n.data(), w.n_inliers, h_n.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_nc.data(), w.rr_consistent, h_nc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_it.data(), w.rr_iters, h_it.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < npairs; i++) {
    const uint8_t s = h_state[(size_t)i];
    state[i] = s;
    if (counts && s < BA_RR_STATES) counts[s]++;
    if (cost) cost[2 * i] = h_cost[(size_t)(2 * i)], cost[2 * i + 1] = h_cost[(size_t)(2 * i + 1)];
    if (iters) iters[i] = h_it[(size_t)i];
    if (s == BA_RR_SKIPPED) continue;  // (its pose, inlier bytes and counts stay as the caller filled them)
    for (int j = 0; j < 6; j++) pose_inout[6 * i + j] = h_pose[(size_t)(6 * i + j)];
    if (inlier_inout)
      for (int64_t k = ptr[(size_t)i]; k < ptr[(size_t)i + 1]; k++) inlier_inout[k] = h_inlier[(size_t)k];
    if (n_inliers) n_inliers[i] = h_n[(size_t)i];
    if (n_consistent) n_consistent[i] = h_nc[(size_t)i];
  }
  return BA_OK;
}

// ---- the homography of a pair: the entries ----------------------------------------------------------------------------
namespace {

// the per-pair buffers of ba_homography and ba_homography_pose, grown for npairs pairs and Hn hypotheses per pair
int homography_buffers(PairWork &w, int64_t npairs, int64_t Hn, bool pose) {
  if (w.hg_cap < npairs) {
    w.hg_cap = 0;
    BA_CHECK(w.hg_H.alloc(HG_DOUBLES * npairs));
    w.hg_cap = npairs;
  }
  if (w.hg_hyp_cap < npairs * Hn) {
    w.hg_hyp_cap = 0;
    BA_CHECK(w.hg_hyp.alloc(HG_DOUBLES * npairs * Hn));
    w.hg_hyp_cap = npairs * Hn;
  }
  if (pose && w.hp_cap < npairs) {
    w.hp_cap = 0;
    BA_CHECK(w.hp_parallax.alloc(npairs));
    BA_CHECK(w.hp_pose.alloc(12 * npairs));
    BA_CHECK(w.hp_normal.alloc(6 * npairs));
    BA_CHECK(w.hp_n.alloc(npairs));
    BA_CHECK(w.hp_support.alloc(2 * npairs));
    w.hp_cap = npairs;
  }
  return BA_OK;
}

}  // namespace

extern "C" int ba_homography(ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                             const ba_ransac_opts *opts, double *H, uint8_t *status, int64_t *match_ptr, uint8_t *inlier,
                             int32_t *n_inliers, int32_t *best_hyp, int64_t *counts) {
  const char *who = "ba_homography";
  ba_ransac_opts o = {};
  if (opts) {
    ba_ransac_opts in = *opts;
    if (in.min_inliers <= 0) in.min_inliers = HG_MIN_INLIERS_DEFAULT;
    if (in.min_inliers < HG_MIN_MATCHES) {
      ba_set_error("%s: min_inliers must be >= %d (<= 0: %d), got %d", who, HG_MIN_MATCHES, HG_MIN_INLIERS_DEFAULT, in.min_inliers);
      return BA_ERR_ARG;
    }
    BA_CHECK(ransac_opts_check(who, &in, &o, HG_MIN_MATCHES, HG_MIN_MATCHES, RN_SAMPLE_MAX));
  }
  if (!p || npairs < 0 || (npairs > 0 && (!x || !pair_a1 || !pair_b1 || !H || !status))) {
    ba_set_error("%s: null argument or npairs < 0", who);
    return BA_ERR_ARG;
  }
  if (p->comm.active()) {
    ba_set_error("%s: not supported on a handle with a communicator (a camera's observations are spread over the shards)", who);
    return BA_ERR_ARG;
  }
  std::vector<int64_t> ptr, oa, ob;
  BA_CHECK(pair_match_lists(who, p->ncams, p->npnts, p->nobs, p->h_cam0.data(), p->h_pnt0.data(), 0, npairs, pair_a1, pair_b1, ptr, &oa, &ob));
  const int64_t nmatch = ptr[(size_t)npairs];
  if (nmatch > (int64_t)INT32_MAX) {
    ba_set_error("%s: %lld matches: more than 2^31 - 1", who, (long long)nmatch);
    return BA_ERR_ARG;
  }
  if (match_ptr)
    for (size_t i = 0; i < ptr.size(); i++) match_ptr[i] = ptr[i];
  if (counts)
    for (int s = 0; s < BA_HG_STATES; s++) counts[s] = 0;
  if (npairs == 0) return BA_OK;
  hipStream_t st = p->stream;
  PairWork &w = p->pairs;
  PairUpload up;
  PairArgs a = {};
  HomArgs q = {};
  const int Hn = opts ? o.hypotheses : 0;
  BA_CHECK(homography_buffers(w, npairs, Hn, false));
  q.hyp_H = w.hg_hyp, q.H = w.hg_H;
  {
    ProfScope ps(p, PC_HOMOGRAPHY, st);
    BA_CHECK(pair_front(p, x, npairs, pair_a1, pair_b1, ptr, oa, ob, Hn, up, a));  // (Hn: the counts of the hypotheses)
    a.hypotheses = Hn, a.sample = o.sample, a.min_inliers = o.min_inliers;
    a.seed_mix = ransac_seed_mix(o.seed), a.tau2 = o.threshold * o.threshold;
    if (opts) BA_CHECK(launch_hom_hypotheses(a, q, npairs, st));
    BA_CHECK(launch_hom_select(a, q, npairs, st));
    for (int it = 0; opts && it < o.refits; it++) BA_CHECK(launch_hom_fit(a, q, npairs, 0, st));
    BA_CHECK(launch_hom_fit(a, q, npairs, 1, st));
  }
  std::vector<double> h_H((size_t)(HG_DOUBLES * npairs));
  std::vector<uint8_t> h_status((size_t)npairs);
  BA_HIP_CHECK(hipMemcpyAsync(h_H.data(), w.hg_H, h_H.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_status.data(), w.status, h_status.size(), hipMemcpyDeviceToHost, st));
  if (inlier && nmatch > 0) BA_HIP_CHECK(hipMemcpyAsync(inlier, w.inlier, (size_t)nmatch, hipMemcpyDeviceToHost, st));
  if (n_inliers) BA_HIP_CHECK(hipMemcpyAsync(n_inliers, w.n_inliers, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (best_hyp) BA_HIP_CHECK(hipMemcpyAsync(best_hyp, w.best_hyp, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < npairs; i++) {
    const uint8_t s = h_status[(size_t)i];
    status[i] = s;
    if (counts && s < BA_HG_STATES) counts[s]++;
    if (s == BA_HG_OK)  // (a pair in any other state leaves its nine entries as the caller filled them)
      for (int j = 0; j < HG_DOUBLES; j++) H[HG_DOUBLES * i + j] = h_H[(size_t)(HG_DOUBLES * i + j)];
  }
  return BA_OK;
}

// the decomposition alone; the handle supplies the device, the stream and the buffers
extern "C" int ba_decompose_homography(ba_problem *p, int64_t n, const double *H, double *R, double *t, double *normal, int32_t *n_sol,
                                       double *parallax) {
  if (!p || n < 0 || (n > 0 && (!H || !R || !t || !normal || !n_sol || !parallax))) {
    ba_set_error("ba_decompose_homography: null argument or n < 0");
    return BA_ERR_ARG;
  }
  if (n > (int64_t)INT32_MAX / 36) {
    ba_set_error("ba_decompose_homography: %lld problems: more than %lld", (long long)n, (long long)(INT32_MAX / 36));
    return BA_ERR_ARG;
  }
  if (n == 0) return BA_OK;
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  PairWork &w = p->pairs;
  if (w.hd_cap < n) {
    w.hd_cap = 0;
    BA_CHECK(w.hd_H.alloc(9 * n));
    BA_CHECK(w.hd_R.alloc(36 * n));
    BA_CHECK(w.hd_t.alloc(12 * n));
    BA_CHECK(w.hd_normal.alloc(12 * n));
    BA_CHECK(w.hd_parallax.alloc(n));
    BA_CHECK(w.hd_n.alloc(n));
    w.hd_cap = n;
  }
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.hd_H, H, (size_t)(9 * n) * sizeof(double), hipMemcpyHostToDevice, st));
  {
    ProfScope ps(p, PC_HOMOGRAPHY, st);
    BA_CHECK(launch_hom_decompose(n, w.hd_H, w.hd_R, w.hd_t, w.hd_normal, w.hd_n, w.hd_parallax, st));
  }
  BA_HIP_CHECK(hipMemcpyAsync(R, w.hd_R, (size_t)(36 * n) * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(t, w.hd_t, (size_t)(12 * n) * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(normal, w.hd_normal, (size_t)(12 * n) * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(n_sol, w.hd_n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(parallax, w.hd_parallax, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

extern "C" int ba_homography_pose(ba_problem *p, const double *x, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                                  const double *H, const uint8_t *status_in, const uint8_t *inlier, double threshold, double *parallax,
                                  int32_t *n_pose, double *pose, double *normal, int32_t *support) {
  const char *who = "ba_homography_pose";
  if (!std::isfinite(threshold) || !(threshold > 0)) {
    ba_set_error("%s: threshold must be finite and > 0 (pixels), got %g", who, threshold);
    return BA_ERR_ARG;
  }
  if (!p || npairs < 0 || (npairs > 0 && (!x || !pair_a1 || !pair_b1 || !H || !inlier || !parallax || !n_pose || !pose))) {
    ba_set_error("%s: null argument or npairs < 0", who);
    return BA_ERR_ARG;
  }
  if (p->comm.active()) {
    ba_set_error("%s: not supported on a handle with a communicator (a camera's observations are spread over the shards)", who);
    return BA_ERR_ARG;
  }
  std::vector<int64_t> ptr, oa, ob;
  BA_CHECK(pair_match_lists(who, p->ncams, p->npnts, p->nobs, p->h_cam0.data(), p->h_pnt0.data(), 0, npairs, pair_a1, pair_b1, ptr, &oa, &ob));
  const int64_t nmatch = ptr[(size_t)npairs];
  if (nmatch > (int64_t)INT32_MAX) {
    ba_set_error("%s: %lld matches: more than 2^31 - 1", who, (long long)nmatch);
    return BA_ERR_ARG;
  }
  if (npairs == 0) return BA_OK;
  hipStream_t st = p->stream;
  PairWork &w = p->pairs;
  PairUpload up;
  PairArgs a = {};
  HomArgs q = {};
  BA_CHECK(homography_buffers(w, npairs, 0, true));
  q.hyp_H = w.hg_hyp, q.H = w.hg_H;
  q.parallax = w.hp_parallax, q.pose2 = w.hp_pose, q.normal2 = w.hp_normal, q.n_pose = w.hp_n, q.support2 = w.hp_support;
  {
    ProfScope ps(p, PC_HOMOGRAPHY, st);
    BA_CHECK(pair_front(p, x, npairs, pair_a1, pair_b1, ptr, oa, ob, 0, up, a));
    a.tau2 = threshold * threshold;
    BA_HIP_CHECK(hipMemcpyAsync((double *)w.hg_H, H, (size_t)(HG_DOUBLES * npairs) * sizeof(double), hipMemcpyHostToDevice, st));
    if (status_in) BA_HIP_CHECK(hipMemcpyAsync((uint8_t *)w.status, status_in, (size_t)npairs, hipMemcpyHostToDevice, st));
    else BA_HIP_CHECK(hipMemsetAsync((uint8_t *)w.status, BA_HG_OK, (size_t)npairs, st));
    if (nmatch > 0) BA_HIP_CHECK(hipMemcpyAsync((uint8_t *)w.inlier, inlier, (size_t)nmatch, hipMemcpyHostToDevice, st));
    BA_CHECK(launch_hom_pose(a, q, npairs, st));
  }
  BA_HIP_CHECK(hipMemcpyAsync(parallax, w.hp_parallax, (size_t)npairs * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(n_pose, w.hp_n, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(pose, w.hp_pose, (size_t)(12 * npairs) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (normal) BA_HIP_CHECK(hipMemcpyAsync(normal, w.hp_normal, (size_t)(6 * npairs) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (support) BA_HIP_CHECK(hipMemcpyAsync(support, w.hp_support, (size_t)(2 * npairs) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}
