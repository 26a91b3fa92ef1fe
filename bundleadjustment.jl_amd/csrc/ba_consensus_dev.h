// The consensus pieces that ba_ransac_cameras and ba_relative_pose share (ba_ransac_kernels.hip, ba_pair_kernels.hip; the rules
// are those of include/ba_hip.h, DESIGN §5m "The consensus stage, written once"): the minimal sample of a hypothesis, the winner
// of a list, the marking of a set and the adopt rule of the refits.  Included inside the including file's unnamed namespace,
// after ba_refine_dev.h (wave_all_sum_int); gfx950 only.  What stays with the callers is what differs: whether a list entry is
// used, the geometry of a hypothesis and the inlier test.
#pragma once

constexpr int CS_BLK = 256, CS_WAVES = CS_BLK / 64;  // the workgroup of every kernel that selects or re-scores

// ---- the sample: lane j holds draw j of the RN_DRAWS of a hypothesis -------------------------------------------------------------
// the list position (< d) of this lane's draw of hypothesis h in a list of d entries
__device__ __forceinline__ int sample_position(uint64_t seed_mix, int h, int lane, int d) {
  return (int)ransac_draw(ransac_mix(seed_mix ^ (uint64_t)h), lane, d);
}

// A draw counts unless its entry is not used or an earlier draw hit its position; the first m that count are the sample.
// take: this lane's draw is of the sample; first: the lane of the first draw that counts (the provisional origin of the sums);
// false: void, fewer than m draws count.  Called by a whole wave; the result is uniform over it.
__device__ __forceinline__ bool sample_take(int pos, bool used, int lane, int m, bool &take, int &first) {
  bool accept = used;
#pragma nounroll
  for (int i = 0; i < RN_DRAWS - 1; i++) {
    const int pi = __shfl(pos, i, 64);
    if (i < lane && pi == pos) accept = false;
  }
  const unsigned long long taken = __ballot(accept);
  if (__popcll(taken) < m) return false;
  take = accept && __popcll(taken & ((1ull << lane) - 1ull)) < m;
  first = __ffsll((long long)taken) - 1;
  return true;
}

// ---- the winner among the H hypotheses of a list -----------------------------------------------------------------------------------
// count[h]: the inliers of hypothesis h, < 0: void.  best: the largest count, ties to the lowest h, -1: none is valid (best_count
// 0).  redk: CS_WAVES entries of LDS.  The key holds count + 1 above 12 bits of h, inverted: the largest key is the largest count
// at the lowest h, 0: no valid hypothesis; the 12 bits are the RN_HYP_MAX of the option check.
__device__ __forceinline__ void consensus_winner(const int *count, int H, int t, long long *redk, int &best, int &best_count) {
  static_assert(RN_HYP_MAX == 1 << 12, "the selection key holds h in 12 bits");
  long long key = 0;
  for (int h = t; h < H; h += CS_BLK) {
    const int cnt = count[h];
    if (cnt >= 0) {
      const long long kk = ((long long)(cnt + 1) << 12) | (long long)(4095 - h);
      key = kk > key ? kk : key;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long other = __shfl_xor(key, off, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) redk[t >> 6] = key;
  __syncthreads();
  for (int w = 0; w < CS_WAVES; w++) key = redk[w] > key ? redk[w] : key;
  best = key ? 4095 - (int)(key & 4095) : -1;
  best_count = key ? (int)(key >> 12) - 1 : 0;
}

// the sum of v over the workgroup -> every thread (red: CS_WAVES ints; a barrier on either side)
__device__ __forceinline__ int block_sum_int(int v, int *red, int t) {
  v = wave_all_sum_int(v);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- the set of a list [k0, k1): one inlier byte per entry, byte_of(k) its index, test(index) the inlier test under a fit ----------
// the set under the fit -> the bytes; returns its size
template <typename At, typename Test>
__device__ __forceinline__ int consensus_mark(int k0, int k1, uint8_t *inlier, int *red, int t, At byte_of, Test test) {
  int n = 0;
  for (int k = k0 + t; k < k1; k += CS_BLK) {
    const int o = byte_of(k);
    const int in = test(o) ? 1 : 0;
    inlier[o] = (uint8_t)in;
    n += in;
  }
  return block_sum_int(n, red, t);
}

// The adopt rule of the refits: M' = the set of the whole list under the new fit, adopted iff |M'| >= |M| = n_old and M' != M;
// otherwise M stays.  Returns |M'| when it was adopted, -1 when not.  Bit 1 of an inlier byte carries M' between the two passes;
// every thread rewrites the bytes it wrote.
template <typename At, typename Test>
__device__ __forceinline__ int consensus_rescore(int k0, int k1, int n_old, uint8_t *inlier, int *red, int t, At byte_of, Test test) {
  int n = 0, diff = 0;
  for (int k = k0 + t; k < k1; k += CS_BLK) {
    const int o = byte_of(k);
    const int in = test(o) ? 1 : 0, old = inlier[o] & 1;
    inlier[o] = (uint8_t)(old | (in << 1));
    n += in;
    diff += in != old ? 1 : 0;
  }
  n = block_sum_int(n, red, t);
  diff = block_sum_int(diff, red, t);
  const bool adopt = n >= n_old && diff > 0;
  for (int k = k0 + t; k < k1; k += CS_BLK) {
    const int o = byte_of(k);
    const int b = inlier[o];
    inlier[o] = (uint8_t)(adopt ? (b >> 1) & 1 : b & 1);
  }
  return adopt ? n : -1;
}
