// The homography of camera pairs (ba_homography, ba_decompose_homography, ba_homography_pose; include/ba_hip.h, "homography of
// camera pairs"): the kernels.  gfx950 only.  The entries, the match lists, the uploads and k_pair_rays are in
// ba_pair_kernels.hip, which launches these kernels through the functions at the end of this file.  They are a unit of their
// own because the kernels of ba_relative_pose are to keep their instructions: with these kernels in their file k_pair_fit came
// out with other registers (tools/compare_code_objects.py against the build before).
// k_pair_hypotheses_h: grid (pair, hypotheses / 4), ONE WAVE PER HYPOTHESIS on its own LDS slab (a PairScratch), the layout of
// k_pair_hypotheses: one draw per lane, the 6 + 45 sums through wave_all_sum, the Jacobi with wave_sync, the sign vote by a
// ballot, and one strided pass over the 40-byte ray records; 9 doubles per hypothesis.
// k_pair_select_h (one workgroup per pair): the states that need no fit, the winner, its inlier bytes.
// k_pair_fit_h (one workgroup per pair): the sums over the set in the fixed order of k_pair_fit (strided partial sums per
// thread, the butterfly of a wave, the four waves in order), the fit, the sign vote, then the re-scoring with the adopt rule
// or, in the last launch, H.
// k_decompose_h: one problem per lane in registers, no LDS.  k_pair_pose_h (one workgroup per pair): the decomposition by one
// lane, the plane votes and the supports by strided counts.
// Every kernel that tests a match under H calls homography_inlier, so a count never disagrees with the bytes; the support of a
// pose is pair_inlier, the test of ba_relative_pose.  No atomics: every output has one writer.
#include <cmath>

#include "ba_internal.h"

namespace {

#include "ba_refine_dev.h"      // wave_all_sum, jacobi12, the pieces of the linear fit, pair_inlier, rotation_vector_reg
#include "ba_consensus_dev.h"   // the sample, the winner, the set and the adopt rule
#include "ba_homography_dev.h"  // the homography: its fit, its inlier test, its decomposition

constexpr int PR_BLK = CS_BLK, PR_WAVES = CS_WAVES;

// (pair_fails, PairFitShared and pair_wave_part of ba_pair_kernels.hip, which keeps its own: they are a few lines)
// a pair that ends here: its state, no inlier, n matches counted, winner h (or -1)
__device__ __forceinline__ void pair_fails(const PairArgs &a, int pr, int k0, int k1, int t, int state, int n, int h) {
  for (int k = k0 + t; k < k1; k += PR_BLK) a.inlier[k] = 0;
  if (t == 0) a.status[pr] = (uint8_t)state, a.n_inliers[pr] = n, a.best_hyp[pr] = h, a.stopped[pr] = 1;
}

// the LDS of k_pair_fit_h: the fit's scratch, the four waves' partial sums, the first match of the set
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

// The linear fit of hypothesis h of a pair -> sh.Rc[0..9); false: void or degenerate.  Called by a whole wave, uniform over it.
__device__ __forceinline__ bool pair_hypothesis_h(const PairArgs &a, PairScratch &sh, const double *in, int h, int k0, int k1, int lane) {
  const int d = k1 - k0, m = a.sample;
  if (d <= 0 || !pair_focals_ok(in)) return false;
  const int pos = sample_position(a.seed_mix, h, lane, d);
  const double *ray = a.rays + PAIR_RAY * (int64_t)(k0 + pos);
  bool take;
  int first;
  if (!sample_take(pos, ray[4] != 0.0, lane, m, take, first)) return false;
  double qax = 0.0, qay = 0.0, qbx = 0.0, qby = 0.0;
  if (take) qax = ray[0], qay = ray[1], qbx = ray[2], qby = ray[3];
  const double oa[2] = {__shfl(qax, first, 64), __shfl(qay, first, 64)}, ob[2] = {__shfl(qbx, first, 64), __shfl(qby, first, 64)};
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
  double da[3] = {0.0, 0.0, 0.0}, db[3] = {0.0, 0.0, 0.0}, acc[EP_SUMS];
  if (take) {
    normalised_ray(qax, qay, oa, dma, sa, da);
    normalised_ray(qbx, qby, ob, dmb, sb, db);
  }
  homography_terms(da, db, acc);
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
  if (!homography_from_sums<wave_sync>(sh, lane, 64, ca, sa, cb, sb)) return false;
  const int front = __popcll(__ballot(take && homography_side(sh.Rc, qax, qay, qbx, qby) > 0.0));
  wave_sync();  // (every lane has read H before lane 0 turns its sign)
  if (lane == 0) homography_sign(sh, front, m);
  wave_sync();
  return true;
}

__global__ __launch_bounds__(PR_BLK) void k_pair_hypotheses_h(PairArgs a, HomArgs q) {
  __shared__ PairScratch shs[PR_WAVES];  // one wave's slab each
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int pr = (int)blockIdx.x, h = (int)blockIdx.y * PR_WAVES + wv;
  if (h >= a.hypotheses) return;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  const int64_t slot = (int64_t)pr * a.hypotheses + h;
  PairScratch &sh = shs[wv];
  int count = -1;
  if (pair_hypothesis_h(a, sh, in, h, k0, k1, lane)) {
    HomMap P;
    homography_map_of(sh.Rc, P);
    count = 0;
    for (int k = k0 + lane; k < k1; k += 64) count += homography_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2) ? 1 : 0;
    count = wave_all_sum_int(count);
    if (lane < HG_DOUBLES) q.hyp_H[HG_DOUBLES * slot + lane] = sh.Rc[lane];
  }
  if (lane == 0) a.hyp_count[slot] = count;
}

// k_pair_select with 4 used matches as the least and the winner's H in place of its pose; the states are BA_HG_*
__global__ __launch_bounds__(PR_BLK) void k_pair_select_h(PairArgs a, HomArgs q) {
  __shared__ long long redk[PR_WAVES];
  __shared__ int red[PR_WAVES];
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  int nu = 0;
  for (int k = k0 + t; k < k1; k += PR_BLK) nu += a.rays[PAIR_RAY * (int64_t)k + 4] != 0.0 ? 1 : 0;
  nu = block_sum_int(nu, red, t);
  if (nu < HG_MIN_MATCHES) return pair_fails(a, pr, k0, k1, t, BA_HG_FEW_MATCHES, 0, -1);
  if (!pair_focals_ok(in)) return pair_fails(a, pr, k0, k1, t, BA_HG_DEGENERATE, 0, -1);
  if (a.hypotheses == 0) {
    for (int k = k0 + t; k < k1; k += PR_BLK) a.inlier[k] = a.rays[PAIR_RAY * (int64_t)k + 4] != 0.0 ? 1 : 0;
    if (t == 0) a.status[pr] = BA_HG_OK, a.n_inliers[pr] = nu, a.best_hyp[pr] = -1, a.stopped[pr] = 0;
    return;
  }
  int best, best_count;
  consensus_winner(a.hyp_count + (int64_t)pr * a.hypotheses, a.hypotheses, t, redk, best, best_count);
  if (best < 0 || best_count < a.min_inliers) return pair_fails(a, pr, k0, k1, t, BA_HG_NO_CONSENSUS, best_count, best);
  HomMap P;
  homography_map_of(q.hyp_H + HG_DOUBLES * ((int64_t)pr * a.hypotheses + best), P);
  const int n = consensus_mark(
      k0, k1, a.inlier, red, t, [](int k) { return k; },
      [&](int k) { return homography_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2); });
  if (t == 0) a.status[pr] = BA_HG_OK, a.n_inliers[pr] = n, a.best_hyp[pr] = best, a.stopped[pr] = 0;
}

// k_pair_fit for the homography: the sums over the set in that kernel's fixed order, the fit, the sign vote over the set; then
// the re-scoring of a refit or, final != 0, H -> q.H or the state DEGENERATE
__global__ __launch_bounds__(PR_BLK) void k_pair_fit_h(PairArgs a, HomArgs q, int final) {
  __shared__ PairFitShared sh;
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  if (a.status[pr] != BA_HG_OK || (!final && a.stopped[pr])) return;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  const int n_old = a.n_inliers[pr];
  PairScratch &ps = sh.ps;
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
        homography_terms(da, db, term);
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
    ok = homography_from_sums<__syncthreads>(ps, t, PR_BLK, ca, sa, cb, sb);
  }
  if (ok) {  // the sign: the matches of the set with d_b' H d_a > 0
    int front = 0;
    for (int k = k0 + t; k < k1; k += PR_BLK)
      if (a.inlier[k] & 1) {
        const double *ray = a.rays + PAIR_RAY * (int64_t)k;
        front += homography_side(ps.Rc, ray[0], ray[1], ray[2], ray[3]) > 0.0 ? 1 : 0;
      }
    front = block_sum_int(front, sh.red, t);
    if (t == 0) homography_sign(ps, front, n_old);
    __syncthreads();
  }
  if (final) {
    if (t == 0 && !ok) a.status[pr] = BA_HG_DEGENERATE;
    if (ok && t < HG_DOUBLES) q.H[HG_DOUBLES * (int64_t)pr + t] = ps.Rc[t];
    return;
  }
  if (!ok) {
    if (t == 0) a.stopped[pr] = 1;
    return;
  }
  HomMap P;
  homography_map_of(ps.Rc, P);
  const int n = consensus_rescore(
      k0, k1, n_old, a.inlier, sh.red, t, [](int k) { return k; },
      [&](int k) { return homography_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2); });
  if (t == 0) {
    if (n >= 0) a.n_inliers[pr] = n;
    else a.stopped[pr] = 1;
  }
}

// ba_decompose_homography: one problem per lane, in registers (homography_decompose is one lane's work), no LDS
__global__ __launch_bounds__(PR_BLK) void k_decompose_h(int64_t n, const double *H, double *R, double *t, double *nrm, int *n_sol,
                                                        double *parallax) {
  const int64_t i = (int64_t)blockIdx.x * PR_BLK + threadIdx.x;
  if (i >= n) return;
  double Hl[9], par;
#pragma unroll
  for (int e = 0; e < 9; e++) Hl[e] = H[9 * i + e];
  n_sol[i] = homography_decompose(Hl, R + 36 * i, t + 12 * i, nrm + 12 * i, par);
  parallax[i] = par;
}

// the LDS of k_pair_pose_h: the four solutions, the kept poses (r, unit t), the counts' scratch
struct HomPoseShared {
  double R[36], t[12], n[12], ret[12], parallax;
  int ns, nk, keep[2], red[PR_WAVES];
};

// One pair per workgroup (ba_homography_pose): thread 0 decomposes the pair's H; every thread counts the matches of the set in
// front of each solution's plane (n' d_a > 0); thread 0 keeps the solutions with more than half of the set, in solver order, at
// most two, and writes (r, unit t, n); then the support of each, the count of pair_inlier over the pair's whole list.
__global__ __launch_bounds__(PR_BLK) void k_pair_pose_h(PairArgs a, HomArgs q) {
  __shared__ HomPoseShared sh;
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  const int k0 = a.match_ptr[pr], k1 = a.match_ptr[pr + 1];
  const double *in = a.intr + 6 * (int64_t)pr;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double *pose = q.pose2 + 12 * (int64_t)pr, *nrm = q.normal2 + 6 * (int64_t)pr;
  if (t < 12) pose[t] = nan;
  if (t < 6) nrm[t] = nan;
  if (t < 2) q.support2[2 * (int64_t)pr + t] = -1;
  if (t == 0) q.n_pose[pr] = 0, q.parallax[pr] = nan;
  if (a.status[pr] != BA_HG_OK || !pair_focals_ok(in)) return;
  if (t == 0) {
    double H[9], par;
#pragma unroll
    for (int e = 0; e < 9; e++) H[e] = q.H[HG_DOUBLES * (int64_t)pr + e];
    sh.ns = homography_decompose(H, sh.R, sh.t, sh.n, par);
    sh.parallax = par;
  }
  __syncthreads();
  const int ns = sh.ns;
  if (ns == 0) return;
  if (ns == 1) {  // a rotation on the spot: its r, no translation, no plane
    if (t == 0) {
      double Rm[9], r[3];
#pragma unroll
      for (int e = 0; e < 9; e++) Rm[e] = sh.R[e];
      rotation_vector_reg(Rm, r);
      pose[0] = r[0], pose[1] = r[1], pose[2] = r[2];
      q.n_pose[pr] = 1, q.parallax[pr] = sh.parallax;
    }
    return;
  }
  int nset = 0, cnt[4] = {0, 0, 0, 0};
  for (int k = k0 + t; k < k1; k += PR_BLK)
    if (a.inlier[k] & 1) {
      const double *ray = a.rays + PAIR_RAY * (int64_t)k;
      nset++;
#pragma unroll
      for (int c = 0; c < 4; c++) cnt[c] += (sh.n[3 * c] * ray[0] + sh.n[3 * c + 1] * ray[1]) - sh.n[3 * c + 2] > 0.0 ? 1 : 0;
    }
  nset = block_sum_int(nset, sh.red, t);
#pragma unroll
  for (int c = 0; c < 4; c++) cnt[c] = block_sum_int(cnt[c], sh.red, t);
  if (t == 0) {
    int nk = 0;
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (2 * cnt[c] > nset && nk < 2) sh.keep[nk++] = c;
    sh.nk = nk;
    for (int j = 0; j < nk; j++) {
      const int c = sh.keep[j];
      double Rm[9], r[3];
#pragma unroll
      for (int e = 0; e < 9; e++) Rm[e] = sh.R[9 * c + e];
      rotation_vector_reg(Rm, r);
      const double t0 = sh.t[3 * c], t1 = sh.t[3 * c + 1], t2 = sh.t[3 * c + 2];
      const double tn = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
      sh.ret[6 * j] = r[0], sh.ret[6 * j + 1] = r[1], sh.ret[6 * j + 2] = r[2];
      sh.ret[6 * j + 3] = t0 / tn, sh.ret[6 * j + 4] = t1 / tn, sh.ret[6 * j + 5] = t2 / tn;
      for (int e = 0; e < 6; e++) pose[6 * j + e] = sh.ret[6 * j + e];
      for (int e = 0; e < 3; e++) nrm[3 * j + e] = sh.n[3 * c + e];
    }
    q.n_pose[pr] = nk, q.parallax[pr] = sh.parallax;
  }
  __syncthreads();
  const int nk = sh.nk;
  for (int j = 0; j < nk; j++) {
    PairPose P;
    pair_pose_of(sh.ret + 6 * j, sh.ret + 6 * j + 3, P);
    int sup = 0;
    for (int k = k0 + t; k < k1; k += PR_BLK) sup += pair_inlier(a.rays + PAIR_RAY * (int64_t)k, P, in[2], in[5], a.tau2) ? 1 : 0;
    sup = block_sum_int(sup, sh.red, t);
    if (t == 0) q.support2[2 * (int64_t)pr + j] = sup;
  }
}

}  // namespace

int launch_hom_hypotheses(const PairArgs &a, const HomArgs &q, int64_t npairs, hipStream_t st) {
  return BA_LAUNCH(k_pair_hypotheses_h, dim3((unsigned)npairs, grid_for(a.hypotheses, PR_WAVES)), PR_BLK, 0, st, a, q);
}

int launch_hom_select(const PairArgs &a, const HomArgs &q, int64_t npairs, hipStream_t st) {
  return BA_LAUNCH(k_pair_select_h, (unsigned)npairs, PR_BLK, 0, st, a, q);
}

int launch_hom_fit(const PairArgs &a, const HomArgs &q, int64_t npairs, int final, hipStream_t st) {
  return BA_LAUNCH(k_pair_fit_h, (unsigned)npairs, PR_BLK, 0, st, a, q, final);
}

int launch_hom_pose(const PairArgs &a, const HomArgs &q, int64_t npairs, hipStream_t st) {
  return BA_LAUNCH(k_pair_pose_h, (unsigned)npairs, PR_BLK, 0, st, a, q);
}

int launch_hom_decompose(int64_t n, const double *H, double *R, double *t, double *normal, int *n_sol, double *parallax, hipStream_t st) {
  return BA_LAUNCH(k_decompose_h, grid_for(n, PR_BLK), PR_BLK, 0, st, n, H, R, t, normal, n_sol, parallax);
}
