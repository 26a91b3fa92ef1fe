// Per-observation 2 x 2 information matrices of the LM solve (ba_lm_set_obs_info, include/ba_hip.h): the whitening
// pass k_info_whiten and the entries that set and read the array of a handle.
//
// Observation i carries Lambda_i = L_i L_i' (L_i lower triangular, factored on the host).  The LM entries minimise
// 1/2 sum_i r_i' Lambda_i r_i (under a robust loss 1/2 sum_i c^2 rho(r_i' Lambda_i r_i / c^2)): with r^_i = L_i' r_i and
// J^_i = L_i' J_i that is the plain problem on r^ and J^.  J^ has the sparsity of J, so everything downstream of the Jacobian
// (the mask, the point and camera blocks, the Schur assembly, the factorisations, PCG, priors, the border, the covariance) runs
// unchanged.  k_info_whiten rewrites r and J in place right after the Jacobian kernel (and the mask); under a robust loss the
// sqrt(w) scaling of k_robust_scale rides in the same pass, from |r^_i|^2, so J is read and written once.
#include <algorithm>
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

constexpr int IB = 256;  // observations per tile = threads per workgroup
constexpr int JV = 12;   // 16-byte vectors of J per observation (2 rows of 12 doubles)
constexpr int JH = 6;    // ... per row

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One tile = IB consecutive observations, streamed as k_robust_scale streams it: thread t handles the residual pair and the
// factor (l00, l10, l11) of observation t, and the tile's 12 IB 16-byte vectors of J are visited by the whole workgroup, vector
// k IB + t by thread t (contiguous 16-byte accesses across the lanes of a wave), all 12 loads of a lane issued before the
// residual's arithmetic.  Vector e of an observation holds columns 2 (e % 6), 2 (e % 6) + 1 of row e / 6, and
//   J^ row 0 = a row 0 + b row 1,   J^ row 1 = c row 1,   (a, b, c) = s (l00, l10, l11),  s = sqrt(w) (1 under the linear loss)
// so a vector of row 0 needs vector e + 6 of the same observation, which another lane holds (12 IB + t has no two members 6
// apart): the row-1 vectors of the tile go through LDS (6 IB vectors, 24 KiB) beside the three factors per observation.
// b == 0 (a diagonal Lambda) leaves row 1 out of row 0 altogether: Lambda = I reproduces J bit for bit.
// J == null: the residual alone (the trial point of the LM loop).  whiten_r: r holds the plain residual (else r^ already: the
// accepted trial residual) -- the loss scaling applies either way.  partial (optional): per-workgroup partials of
// sum c^2 rho(z) and of |r~|^2 in the layout, grid and tree of k_robust_scale.  440 bytes per observation in all.
// Built without FMA contraction (Makefile): r^ = (l00 r_x + l10 r_y, l11 r_y) and |r^|^2 round as written.
template <int KIND, bool WEIGHTS>
__global__ __launch_bounds__(IB) void k_info_whiten(int64_t nobs, double c2, const double *__restrict__ L, double2 *__restrict__ r,
                                                    double2 *__restrict__ J, double *__restrict__ wout,
                                                    double *__restrict__ partial, int whiten_r) {
  __shared__ double2 srow1[IB * JH];
  __shared__ double sf[3][IB];
  __shared__ double red[2][IB / 64];
  const int t = threadIdx.x;
  const int64_t ntile = (nobs + IB - 1) / IB, nJ = nobs * JV;
  const bool jac = J != nullptr;  // (uniform)
  double acc_c = 0, acc_r = 0;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t o = tile * IB + t, j0 = tile * IB * JV;
    double2 jv[JV];
    if (jac) {
#pragma unroll
      for (int k = 0; k < JV; k++) {
        const int64_t q = j0 + k * IB + t;
        jv[k] = q < nJ ? J[q] : make_double2(0.0, 0.0);
      }
    }
    double a = 1.0, b = 0.0, c = 1.0;
    if (o < nobs) {
      const double l00 = L[3 * o], l10 = L[3 * o + 1], l11 = L[3 * o + 2];
      double2 e = r[o];
      if (whiten_r) {
        e.x = l00 * e.x;
        if (l10 != 0.0) e.x += l10 * e.y;
        e.y = l11 * e.y;
      }
      double w;
      acc_c += robust_rho(KIND, e.x * e.x + e.y * e.y, c2, &w);
      a = l00, b = l10, c = l11;
      if (KIND != BA_LOSS_LINEAR) {
        const double s = sqrt(w);
        e.x *= s;
        e.y *= s;
        a *= s, b *= s, c *= s;
      }
      if (KIND != BA_LOSS_LINEAR || whiten_r) r[o] = e;
      acc_r += e.x * e.x + e.y * e.y;
      if (WEIGHTS) wout[o] = w;
    }
    if (jac) {
      sf[0][t] = a;
      sf[1][t] = b;
      sf[2][t] = c;
#pragma unroll
      for (int k = 0; k < JV; k++) {
        const int v = k * IB + t, e = v % JV;
        if (e >= JH) srow1[(v / JV) * JH + (e - JH)] = jv[k];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < JV; k++) {
        const int v = k * IB + t;
        const int64_t q = j0 + v;
        if (q < nJ) {
          const int ol = v / JV, e = v % JV;
          double2 out = jv[k];
          if (e < JH) {
            const double fa = sf[0][ol], fb = sf[1][ol];
            out.x *= fa;
            out.y *= fa;
            if (fb != 0.0) {
              const double2 p1 = srow1[ol * JH + e];
              out.x += fb * p1.x;
              out.y += fb * p1.y;
            }
          } else {
            const double fc = sf[2][ol];
            out.x *= fc;
            out.y *= fc;
          }
          J[q] = out;
        }
      }
      __syncthreads();  // sf and srow1 are rewritten by the next tile
    }
  }
  if (partial == nullptr) return;  // (uniform)
  acc_c = wave_sum(acc_c);
  acc_r = wave_sum(acc_r);
  if ((t & 63) == 0) {
    red[0][t >> 6] = acc_c;
    red[1][t >> 6] = acc_r;
  }
  __syncthreads();
  if (t == 0) {
    partial[blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    partial[RED_BLOCKS + blockIdx.x] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

template <int KIND>
void launch_kind(int nb, hipStream_t st, int64_t nobs, double c2, const double *d_L, double *d_r, double *d_J, double *d_w,
                 double *d_partial, int whiten_r) {
  if (d_w)
    hipLaunchKernelGGL((k_info_whiten<KIND, true>), dim3(nb), dim3(IB), 0, st, nobs, c2, d_L, (double2 *)d_r, (double2 *)d_J, d_w,
                       d_partial, whiten_r);
  else
    hipLaunchKernelGGL((k_info_whiten<KIND, false>), dim3(nb), dim3(IB), 0, st, nobs, c2, d_L, (double2 *)d_r, (double2 *)d_J,
                       (double *)nullptr, d_partial, whiten_r);
}

}  // namespace

// the handle's factors to the device, once per change (ba_lm_set_obs_info marks them dirty).  The buffer is allocated at its
// full size at the first upload and never reallocated; a handle whose array is cleared keeps it (unused).
int info_upload(ba_problem *p) {
  if (!p->info_dirty) return BA_OK;
  if (p->info_on()) {
    if (!p->d_info) BA_CHECK(p->d_info.alloc(3 * p->nobs));
    if (p->nobs > 0)
      BA_HIP_CHECK(hipMemcpyAsync(p->d_info, p->h_info.data(), (size_t)(3 * p->nobs) * sizeof(double), hipMemcpyHostToDevice,
                                  p->stream));
    BA_HIP_CHECK(hipStreamSynchronize(p->stream));  // (the host array may change with the next ba_lm_set_obs_info)
  }
  p->info_dirty = false;
  return BA_OK;
}

int launch_info_whiten(ba_problem *p, double *d_r, double *d_J, double *d_w, double *d_partial, bool residual_plain,
                       bool with_loss, hipStream_t st) {
  if (!p->info_on() || p->nobs <= 0) return BA_OK;
  ProfScope ps(p, PC_INFO, st);
  const int nb = robust_blocks(p->nobs);
  const double c2 = p->loss_scale * p->loss_scale;
  const double *L = p->d_info;
  const int wr = residual_plain ? 1 : 0;
  switch (with_loss ? p->loss : BA_LOSS_LINEAR) {
    case BA_LOSS_HUBER: launch_kind<BA_LOSS_HUBER>(nb, st, p->nobs, c2, L, d_r, d_J, d_w, d_partial, wr); break;
    case BA_LOSS_SOFT_L1: launch_kind<BA_LOSS_SOFT_L1>(nb, st, p->nobs, c2, L, d_r, d_J, d_w, d_partial, wr); break;
    case BA_LOSS_CAUCHY: launch_kind<BA_LOSS_CAUCHY>(nb, st, p->nobs, c2, L, d_r, d_J, d_w, d_partial, wr); break;
    case BA_LOSS_ARCTAN: launch_kind<BA_LOSS_ARCTAN>(nb, st, p->nobs, c2, L, d_r, d_J, d_w, d_partial, wr); break;
    default: launch_kind<BA_LOSS_LINEAR>(nb, st, p->nobs, c2, L, d_r, d_J, d_w, d_partial, wr); break;
  }
  BA_HIP_CHECK(hipGetLastError());
  return BA_OK;
}

extern "C" int ba_lm_set_obs_info(ba_problem *p, const double *info3) {
  if (!p) {
    ba_set_error("ba_lm_set_obs_info: null handle");
    return BA_ERR_ARG;
  }
  if (!info3) {
    p->h_info.clear();
    p->info_set = false;
    p->info_zero = 0;
    p->info_dirty = false;
    return BA_OK;
  }
  std::vector<double> f((size_t)(3 * p->nobs));
  int64_t nzero = 0;
  for (int64_t o = 0; o < p->nobs; o++) {
    const double xx = info3[3 * o], xy = info3[3 * o + 1], yy = info3[3 * o + 2];
    if (!std::isfinite(xx) || !std::isfinite(xy) || !std::isfinite(yy)) {
      ba_set_error("ba_lm_set_obs_info: observation %lld: the information matrix must be finite, got (%g, %g, %g)", (long long)o,
                   xx, xy, yy);
      return BA_ERR_ARG;
    }
    if (xx < 0 || yy < 0) {
      ba_set_error("ba_lm_set_obs_info: observation %lld: negative diagonal entry (xx %g, yy %g)", (long long)o, xx, yy);
      return BA_ERR_ARG;
    }
    if (xy * xy > xx * yy) {
      ba_set_error("ba_lm_set_obs_info: observation %lld: not positive semi-definite (xy^2 = %g > xx yy = %g)", (long long)o,
                   xy * xy, xx * yy);
      return BA_ERR_ARG;
    }
    const double l00 = std::sqrt(xx), l10 = xx > 0 ? xy / l00 : 0.0, l11 = std::sqrt(std::max(yy - l10 * l10, 0.0));
    f[(size_t)(3 * o)] = l00;
    f[(size_t)(3 * o + 1)] = l10;
    f[(size_t)(3 * o + 2)] = l11;
    if (xx == 0 && xy == 0 && yy == 0) nzero++;
  }
  // (no workspace is touched here: the array may be set before or after the first solve)
  p->h_info.swap(f);
  p->info_set = true;
  p->info_zero = nzero;
  p->info_version++;
  p->info_dirty = true;
  return BA_OK;
}

extern "C" int ba_lm_get_obs_info(const ba_problem *p, int64_t *n_set, int64_t *n_zero) {
  if (!p) {
    ba_set_error("ba_lm_get_obs_info: null handle");
    return BA_ERR_ARG;
  }
  if (n_set) *n_set = p->info_set ? p->nobs : 0;
  if (n_zero) *n_zero = p->info_set ? p->info_zero : 0;
  return BA_OK;
}
