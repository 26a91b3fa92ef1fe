// The similarity alignment of reconstructions (ba_similarity; include/ba_hip.h, "similarity alignment"): the kernels and
// the entry.  gfx950 only.  A unit of its own, as ba_homography_kernels.hip is, so that the kernels of the other consensus users
// keep their instructions (tools/compare_code_objects.py against the build before).
// A row of a problem is one record of SM_ROW doubles (src, dst, used), packed on the host and uploaded once.
// k_similarity_hypotheses: grid (problem, hypotheses / 4), ONE WAVE PER HYPOTHESIS, the layout of k_pair_hypotheses_h: one draw per
// lane, the 16 sums through wave_all_sum, the closed form in the registers of every lane (the same bits in each), and one strided
// pass over the problem's records for the count; 13 doubles (s, R, t) per hypothesis.
// k_similarity_select (one workgroup per problem): the states that need no fit, the winner, its inlier bytes.
// k_similarity_fit (one workgroup per problem): the lowest index of the set, the 16 sums over the set in the fixed order of
// k_pair_fit_h (strided partial sums per thread, the butterfly of a wave, the four waves in order), the fit, then the re-scoring
// with the adopt rule or, in the last launch, sim, rms and the state.
// Every kernel that tests a row under a fit calls similarity_inlier, so a count never disagrees with the bytes.  No atomics: every
// output has one writer.
#include <cmath>

#include "ba_internal.h"

namespace {

#include "ba_refine_dev.h"      // wave_all_sum, rotation_vector_reg, RS_SWEEPS
#include "ba_consensus_dev.h"   // the sample, the winner, the set and the adopt rule
#include "ba_similarity_dev.h"  // the similarity: its fit and its inlier test

constexpr int SM_BLK = CS_BLK, SM_WAVES = CS_WAVES;

// a problem that ends here: its state, no inlier, n rows counted, winner h (or -1)
__device__ __forceinline__ void similarity_fails(const SimArgs &a, int pr, int k0, int k1, int t, int state, int n, int h) {
  for (int k = k0 + t; k < k1; k += SM_BLK) a.inlier[k] = 0;
  if (t == 0) a.status[pr] = (uint8_t)state, a.n_inliers[pr] = n, a.best_hyp[pr] = h, a.stopped[pr] = 1;
}

// the LDS of k_similarity_fit: the four waves' partial sums, the sums, the lowest index of the set and the counts' scratch
struct SimFitShared {
  double part[SM_WAVES][SM_SUMS];
  double S[SM_SUMS];
  int red[SM_WAVES];
};

// The fit of hypothesis h of a problem -> P; false: void or degenerate.  Called by a whole wave, uniform over it.
__device__ __forceinline__ bool similarity_hypothesis(const SimArgs &a, int h, int k0, int k1, int lane, double P[SM_FIT]) {
  const int d = k1 - k0, m = a.sample;
  if (d <= 0) return false;
  const int pos = sample_position(a.seed_mix, h, lane, d);
  const double *row = a.rows + SM_ROW * (int64_t)(k0 + pos);
  bool take;
  int first;
  if (!sample_take(pos, row[6] != 0.0, lane, m, take, first)) return false;
  double so[3], dq[3];
#pragma unroll
  for (int i = 0; i < 3; i++) so[i] = __shfl(row[i], first, 64), dq[i] = __shfl(row[3 + i], first, 64);
  double S[SM_SUMS];
#pragma unroll
  for (int i = 0; i < SM_SUMS; i++) S[i] = 0.0;
  if (take) similarity_terms(row, so, dq, S);
#pragma unroll
  for (int i = 0; i < SM_SUMS; i++) S[i] = wave_all_sum(S[i]);
  return similarity_from_sums(S, (double)m, so, dq, a.with_scale, P);
}

__global__ __launch_bounds__(SM_BLK) void k_similarity_hypotheses(SimArgs a) {
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int pr = (int)blockIdx.x, h = (int)blockIdx.y * SM_WAVES + wv;
  if (h >= a.hypotheses) return;
  const int k0 = a.row_ptr[pr], k1 = a.row_ptr[pr + 1];
  const int64_t slot = (int64_t)pr * a.hypotheses + h;
  double P[SM_FIT];
  int count = -1;
  if (similarity_hypothesis(a, h, k0, k1, lane, P)) {
    count = 0;
    for (int k = k0 + lane; k < k1; k += 64) count += similarity_inlier(a.rows + SM_ROW * (int64_t)k, P, a.tau2) ? 1 : 0;
    count = wave_all_sum_int(count);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < SM_FIT; e++) a.hyp[SM_FIT * slot + e] = P[e];
    }
  }
  if (lane == 0) a.hyp_count[slot] = count;
}

// the states that need no fit, the winner among the hypotheses and its set
__global__ __launch_bounds__(SM_BLK) void k_similarity_select(SimArgs a) {
  __shared__ long long redk[SM_WAVES];
  __shared__ int red[SM_WAVES];
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  const int k0 = a.row_ptr[pr], k1 = a.row_ptr[pr + 1];
  int nu = 0;
  for (int k = k0 + t; k < k1; k += SM_BLK) nu += a.rows[SM_ROW * (int64_t)k + 6] != 0.0 ? 1 : 0;
  nu = block_sum_int(nu, red, t);
  if (nu < SM_MIN_ROWS) return similarity_fails(a, pr, k0, k1, t, BA_SM_FEW_ROWS, 0, -1);
  if (a.hypotheses == 0) {
    for (int k = k0 + t; k < k1; k += SM_BLK) a.inlier[k] = a.rows[SM_ROW * (int64_t)k + 6] != 0.0 ? 1 : 0;
    if (t == 0) a.status[pr] = BA_SM_OK, a.n_inliers[pr] = nu, a.best_hyp[pr] = -1, a.stopped[pr] = 0;
    return;
  }
  int best, best_count;
  consensus_winner(a.hyp_count + (int64_t)pr * a.hypotheses, a.hypotheses, t, redk, best, best_count);
  if (best < 0 || best_count < a.min_inliers) return similarity_fails(a, pr, k0, k1, t, BA_SM_NO_CONSENSUS, best_count, best);
  double P[SM_FIT];
#pragma unroll
  for (int e = 0; e < SM_FIT; e++) P[e] = a.hyp[SM_FIT * ((int64_t)pr * a.hypotheses + best) + e];
  const int n = consensus_mark(
      k0, k1, a.inlier, red, t, [](int k) { return k; }, [&](int k) { return similarity_inlier(a.rows + SM_ROW * (int64_t)k, P, a.tau2); });
  if (t == 0) a.status[pr] = BA_SM_OK, a.n_inliers[pr] = n, a.best_hyp[pr] = best, a.stopped[pr] = 0;
}

// The fit on the set: the sums about the set's first row in the fixed order of k_pair_fit_h, the closed form in every thread's
// registers; then the re-scoring of a refit or, final != 0, (s, r, t) -> a.sim with the rms over the set, or the state DEGENERATE
__global__ __launch_bounds__(SM_BLK) void k_similarity_fit(SimArgs a, int final) {
  __shared__ SimFitShared sh;
  const int t = (int)threadIdx.x, pr = (int)blockIdx.x;
  if (a.status[pr] != BA_SM_OK || (!final && a.stopped[pr])) return;
  const int k0 = a.row_ptr[pr], k1 = a.row_ptr[pr + 1];
  const int n_old = a.n_inliers[pr];
  int first = k1;
  for (int k = k0 + t; k < k1; k += SM_BLK)
    if ((a.inlier[k] & 1) && k < first) first = k;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int other = __shfl_xor(first, off, 64);
    first = other < first ? other : first;
  }
  if ((t & 63) == 0) sh.red[t >> 6] = first;
  __syncthreads();
  for (int w = 0; w < SM_WAVES; w++) first = sh.red[w] < first ? sh.red[w] : first;
  __syncthreads();              // (sh.red is written again below)
  bool ok = first < k1;         // (every decision below is taken on values all threads share)
  double P[SM_FIT];
  if (ok) {
    const double *r0 = a.rows + SM_ROW * (int64_t)first;
    const double so[3] = {r0[0], r0[1], r0[2]}, dq[3] = {r0[3], r0[4], r0[5]};
    double acc[SM_SUMS];
#pragma unroll
    for (int i = 0; i < SM_SUMS; i++) acc[i] = 0.0;
    for (int k = k0 + t; k < k1; k += SM_BLK)
      if (a.inlier[k] & 1) {
        double term[SM_SUMS];
        similarity_terms(a.rows + SM_ROW * (int64_t)k, so, dq, term);
#pragma unroll
        for (int i = 0; i < SM_SUMS; i++) acc[i] += term[i];
      }
#pragma unroll
    for (int i = 0; i < SM_SUMS; i++) {
      const double v = wave_all_sum(acc[i]);
      if ((t & 63) == 0) sh.part[t >> 6][i] = v;
    }
    __syncthreads();
    if (t < SM_SUMS) sh.S[t] = ((sh.part[0][t] + sh.part[1][t]) + sh.part[2][t]) + sh.part[3][t];
    __syncthreads();
    double S[SM_SUMS];
#pragma unroll
    for (int i = 0; i < SM_SUMS; i++) S[i] = sh.S[i];
    ok = similarity_from_sums(S, (double)n_old, so, dq, a.with_scale, P);
  }
  if (final) {
    if (!ok) {
      if (t == 0) a.status[pr] = BA_SM_DEGENERATE;
      return;
    }
    double e2 = 0.0;
    for (int k = k0 + t; k < k1; k += SM_BLK)
      if (a.inlier[k] & 1) e2 += similarity_residual2(a.rows + SM_ROW * (int64_t)k, P);
    e2 = wave_all_sum(e2);
    __syncthreads();  // (every thread has read sh.S)
    if ((t & 63) == 0) sh.S[t >> 6] = e2;
    __syncthreads();
    if (t == 0) {
      double r[3];
      rotation_vector_reg(P + 1, r);
      double *out = a.sim + 7 * (int64_t)pr;
      out[0] = P[0], out[1] = r[0], out[2] = r[1], out[3] = r[2], out[4] = P[10], out[5] = P[11], out[6] = P[12];
      a.rms[pr] = sqrt((((sh.S[0] + sh.S[1]) + sh.S[2]) + sh.S[3]) / (double)n_old);
    }
    return;
  }
  if (!ok) {
    if (t == 0) a.stopped[pr] = 1;
    return;
  }
  const int n = consensus_rescore(
      k0, k1, n_old, a.inlier, sh.red, t, [](int k) { return k; },
      [&](int k) { return similarity_inlier(a.rows + SM_ROW * (int64_t)k, P, a.tau2); });
  if (t == 0) {
    if (n >= 0) a.n_inliers[pr] = n;
    else a.stopped[pr] = 1;
  }
}

}  // namespace

extern "C" int ba_similarity(ba_problem *p, int64_t nprob, const int64_t *row_ptr, const double *src, const double *dst, const uint8_t *used,
                             const ba_ransac_opts *opts, int with_scale, double *sim, uint8_t *status, uint8_t *inlier, int32_t *n_inliers,
                             int32_t *best_hyp, double *rms, int64_t *counts) {
  const char *who = "ba_similarity";
  ba_ransac_opts o = {};
  if (opts) {
    if (!std::isfinite(opts->threshold) || !(opts->threshold > 0)) {
      ba_set_error("%s: threshold must be finite and > 0 (the units of dst), got %g", who, opts->threshold);
      return BA_ERR_ARG;
    }
    BA_CHECK(ransac_opts_check(who, opts, &o, SM_MIN_ROWS, SM_MIN_ROWS, RN_SAMPLE_MAX));
  }
  if (!p || nprob < 0 || (nprob > 0 && (!row_ptr || !sim || !status))) {
    ba_set_error("%s: null argument or nprob < 0", who);
    return BA_ERR_ARG;
  }
  if (p->comm.active()) {
    ba_set_error("%s: not supported on a handle with a communicator (several ranks are out of scope)", who);
    return BA_ERR_ARG;
  }
  if (counts)
    for (int s = 0; s < BA_SM_STATES; s++) counts[s] = 0;
  if (nprob == 0) return BA_OK;
  if (row_ptr[0] != 0) {
    ba_set_error("%s: row_ptr must start at 0, got %lld", who, (long long)row_ptr[0]);
    return BA_ERR_ARG;
  }
  for (int64_t k = 0; k < nprob; k++)
    if (row_ptr[k + 1] < row_ptr[k]) {
      ba_set_error("%s: row_ptr must not decrease, got %lld after %lld at problem %lld", who, (long long)row_ptr[k + 1], (long long)row_ptr[k],
                   (long long)k);
      return BA_ERR_ARG;
    }
  const int64_t n = row_ptr[nprob];
  if (n > (int64_t)INT32_MAX) {
    ba_set_error("%s: %lld rows: more than 2^31 - 1", who, (long long)n);
    return BA_ERR_ARG;
  }
  if (n > 0 && (!src || !dst)) {
    ba_set_error("%s: null argument (src or dst)", who);
    return BA_ERR_ARG;
  }
  // the row records: a row is used iff its byte says so and its six numbers are finite
  std::vector<double> rows((size_t)(SM_ROW * n));
  for (int64_t k = 0; k < n; k++) {
    double *row = rows.data() + SM_ROW * k;
    bool fin = true;
    for (int i = 0; i < 3; i++) {
      row[i] = src[3 * k + i], row[3 + i] = dst[3 * k + i];
      fin = fin && std::isfinite(row[i]) && std::isfinite(row[3 + i]);
    }
    row[6] = fin && (!used || used[k]) ? 1.0 : 0.0;
  }
  std::vector<int> ptr((size_t)nprob + 1);
  for (int64_t k = 0; k <= nprob; k++) ptr[(size_t)k] = (int)row_ptr[k];
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  SimilarityWork &w = p->similarity;
  const int Hn = opts ? o.hypotheses : 0;
  BA_CHECK(put(w.row_ptr, ptr, st));
  BA_CHECK(put(w.rows, rows, st));
  BA_CHECK(grow(w.hyp, SM_FIT * nprob * Hn));
  BA_CHECK(grow(w.hyp_count, nprob * Hn));
  BA_CHECK(grow(w.inlier, n));
  for (GrowBuf<uint8_t> *b : {&w.stopped, &w.status}) BA_CHECK(grow(*b, nprob));
  for (GrowBuf<int> *b : {&w.n_inliers, &w.best_hyp}) BA_CHECK(grow(*b, nprob));
  BA_CHECK(grow(w.sim, 7 * nprob));
  BA_CHECK(grow(w.rms, nprob));
  SimArgs a = {};
  a.row_ptr = w.row_ptr, a.rows = w.rows, a.hyp = w.hyp, a.hyp_count = w.hyp_count;
  a.inlier = w.inlier, a.stopped = w.stopped, a.status = w.status, a.n_inliers = w.n_inliers, a.best_hyp = w.best_hyp;
  a.sim = w.sim, a.rms = w.rms;
  a.hypotheses = Hn, a.sample = o.sample, a.min_inliers = o.min_inliers, a.with_scale = with_scale ? 1 : 0;
  a.seed_mix = ransac_seed_mix(o.seed), a.tau2 = o.threshold * o.threshold;
  {
    ProfScope ps(p, PC_SIMILARITY, st);
    if (opts) BA_CHECK(BA_LAUNCH(k_similarity_hypotheses, dim3((unsigned)nprob, grid_for(Hn, SM_WAVES)), SM_BLK, 0, st, a));
    BA_CHECK(BA_LAUNCH(k_similarity_select, (unsigned)nprob, SM_BLK, 0, st, a));
    for (int it = 0; opts && it < o.refits; it++) BA_CHECK(BA_LAUNCH(k_similarity_fit, (unsigned)nprob, SM_BLK, 0, st, a, 0));
    BA_CHECK(BA_LAUNCH(k_similarity_fit, (unsigned)nprob, SM_BLK, 0, st, a, 1));
  }
  std::vector<double> h_sim((size_t)(7 * nprob)), h_rms((size_t)nprob);
  std::vector<uint8_t> h_status((size_t)nprob);
  BA_HIP_CHECK(hipMemcpyAsync(h_sim.data(), w.sim, h_sim.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_rms.data(), w.rms, h_rms.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(h_status.data(), w.status, h_status.size(), hipMemcpyDeviceToHost, st));
  if (inlier && n > 0) BA_HIP_CHECK(hipMemcpyAsync(inlier, w.inlier, (size_t)n, hipMemcpyDeviceToHost, st));
  if (n_inliers) BA_HIP_CHECK(hipMemcpyAsync(n_inliers, w.n_inliers, (size_t)nprob * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (best_hyp) BA_HIP_CHECK(hipMemcpyAsync(best_hyp, w.best_hyp, (size_t)nprob * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < nprob; i++) {
    const uint8_t s = h_status[(size_t)i];
    status[i] = s;
    if (counts && s < BA_SM_STATES) counts[s]++;
    if (rms) rms[i] = s == BA_SM_OK ? h_rms[(size_t)i] : std::nan("");
    if (s == BA_SM_OK)  // (a problem in any other state leaves its seven entries as the caller filled them)
      for (int j = 0; j < 7; j++) sim[7 * i + j] = h_sim[(size_t)(7 * i + j)];
  }
  return BA_OK;
}
