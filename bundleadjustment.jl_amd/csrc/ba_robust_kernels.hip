// Robust loss of the LM solve (ba_lm_set_loss, include/ba_hip.h): the per-observation reweighting pass k_robust_scale and
// the entries that set, read and evaluate the loss of a handle.
//
// The LM loop linearises f(x) = 1/2 sum_i c^2 rho(|r_i|^2 / c^2) in the first-order (IRLS) form: r~_i = sqrt(w_i) r_i,
// J~_i = sqrt(w_i) J_i with w_i = rho'(z_i).  J~'J~ has the sparsity of J'J, so everything downstream of the Jacobian (the
// point and camera blocks, the Schur assembly, the factorisations, PCG, the sharded path) runs unchanged on J~ and r~.
// k_robust_scale rewrites r and J in place right after the Jacobian kernel and leaves nothing per observation behind.
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

constexpr int RB = 256;  // observations per tile = threads per workgroup
constexpr int JV = 12;   // 16-byte vectors of J per observation (2 x 12 doubles)

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One tile = RB consecutive observations: thread t reweights the residual pair of observation t (one 16-byte load and store)
// and puts sqrt(w) in LDS; then the tile's 12 RB 16-byte vectors of J are streamed by the whole workgroup, vector k RB + t by
// thread t -- contiguous 16-byte accesses across the lanes of a wave, the vector's observation (k RB + t) / 12 read from LDS.
// The loads of J are issued before the residual's arithmetic (12 vectors in flight per lane).  416 bytes per observation in
// all.  Workgroups stride over the tiles; the grid depends on nobs only, so the partial sums (cost and |r~|^2, one per
// workgroup, in a fixed tree) do too.  One instantiation per loss: only its own rho stays live beside the 12 vectors of J.
template <int KIND, bool WEIGHTS>
__global__ __launch_bounds__(RB) void k_robust_scale(int64_t nobs, double c2, double2 *__restrict__ r,
                                                     double2 *__restrict__ J, double *__restrict__ wout,
                                                     double *__restrict__ partial) {
  __shared__ double sw[RB];
  __shared__ double red[2][RB / 64];
  const int t = threadIdx.x;
  const int64_t ntile = (nobs + RB - 1) / RB, nJ = nobs * JV;
  double acc_c = 0, acc_r = 0;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t o = tile * RB + t, j0 = tile * RB * JV;
    double2 jv[JV];
#pragma unroll
    for (int k = 0; k < JV; k++) {
      const int64_t q = j0 + k * RB + t;
      jv[k] = q < nJ ? J[q] : make_double2(0.0, 0.0);
    }
    double s = 1.0;
    if (o < nobs) {
      double2 e = r[o];
      double w;
      acc_c += robust_rho(KIND, e.x * e.x + e.y * e.y, c2, &w);
      s = sqrt(w);
      e.x *= s;
      e.y *= s;
      r[o] = e;
      acc_r += e.x * e.x + e.y * e.y;
      if (WEIGHTS) wout[o] = w;
    }
    sw[t] = s;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < JV; k++) {
      const int64_t q = j0 + k * RB + t;
      if (q < nJ) {
        const double f = sw[(k * RB + t) / JV];
        jv[k].x *= f;
        jv[k].y *= f;
        J[q] = jv[k];
      }
    }
    __syncthreads();  // sw is rewritten by the next tile
  }
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
void launch_kind(int nb, hipStream_t st, int64_t nobs, double c2, double *d_r, double *d_J, double *d_w, double *d_partial) {
  if (d_w)
    hipLaunchKernelGGL((k_robust_scale<KIND, true>), dim3(nb), dim3(RB), 0, st, nobs, c2, (double2 *)d_r, (double2 *)d_J, d_w,
                       d_partial);
  else
    hipLaunchKernelGGL((k_robust_scale<KIND, false>), dim3(nb), dim3(RB), 0, st, nobs, c2, (double2 *)d_r, (double2 *)d_J,
                       (double *)nullptr, d_partial);
}

}  // namespace

int robust_blocks(int64_t nobs) {
  const int64_t ntile = (nobs + RB - 1) / RB;
  return (int)(ntile < 1 ? 1 : (ntile > RED_BLOCKS ? RED_BLOCKS : ntile));
}

int launch_robust_scale(ba_problem *p, double *d_r, double *d_J, double *d_w, double *d_partial, hipStream_t st) {
  ProfScope ps(p, PC_ROBUST, st);
  const int nb = robust_blocks(p->nobs);
  const double c2 = p->loss_scale * p->loss_scale;
  switch (p->loss) {
    case BA_LOSS_HUBER: launch_kind<BA_LOSS_HUBER>(nb, st, p->nobs, c2, d_r, d_J, d_w, d_partial); break;
    case BA_LOSS_SOFT_L1: launch_kind<BA_LOSS_SOFT_L1>(nb, st, p->nobs, c2, d_r, d_J, d_w, d_partial); break;
    case BA_LOSS_CAUCHY: launch_kind<BA_LOSS_CAUCHY>(nb, st, p->nobs, c2, d_r, d_J, d_w, d_partial); break;
    case BA_LOSS_ARCTAN: launch_kind<BA_LOSS_ARCTAN>(nb, st, p->nobs, c2, d_r, d_J, d_w, d_partial); break;
    default: launch_kind<BA_LOSS_LINEAR>(nb, st, p->nobs, c2, d_r, d_J, d_w, d_partial); break;
  }
  BA_HIP_CHECK(hipGetLastError());
  return BA_OK;
}

extern "C" int ba_lm_set_loss(ba_problem *p, int kind, double scale) {
  if (!p) {
    ba_set_error("ba_lm_set_loss: null handle");
    return BA_ERR_ARG;
  }
  if (kind < BA_LOSS_LINEAR || kind > BA_LOSS_ARCTAN) {
    ba_set_error("ba_lm_set_loss: unknown loss kind %d (0 linear, 1 huber, 2 soft_l1, 3 cauchy, 4 arctan)", kind);
    return BA_ERR_ARG;
  }
  if (!(scale > 0) || !std::isfinite(scale)) {
    ba_set_error("ba_lm_set_loss: the scale (f_scale) must be finite and > 0, got %g", scale);
    return BA_ERR_ARG;
  }
  p->loss = kind;
  p->loss_scale = scale;
  return BA_OK;
}

extern "C" int ba_lm_get_loss(const ba_problem *p, int *kind, double *scale) {
  if (!p) {
    ba_set_error("ba_lm_get_loss: null handle");
    return BA_ERR_ARG;
  }
  if (kind) *kind = p->loss;
  if (scale) *scale = p->loss_scale;
  return BA_OK;
}

// r and J at x, k_robust_scale with the weights written out, the cost partials summed by the fixed tree of the LM loop; with
// per-observation information on the handle (ba_lm_set_obs_info) k_info_whiten in its place: w and f of r' Lambda r
extern "C" int ba_robust_eval(ba_problem *p, const double *x, double *weights, double *cost) {
  if (!p || !x) {
    ba_set_error("ba_robust_eval: null argument");
    return BA_ERR_ARG;
  }
  BA_HIP_CHECK(hipSetDevice(p->device));
  BA_CHECK(info_upload(p));
  const int64_t nvar = 9 * p->ncams + 3 * p->npnts, nobs = p->nobs;
  hipStream_t st = p->stream;
  double *dx, *dr, *dJ, *dw;
  BA_CHECK(ba_scratch(p, 0, (size_t)(nvar + 1) * sizeof(double), (void **)&dx));
  BA_CHECK(ba_scratch(p, 1, (size_t)(2 * nobs + 2) * sizeof(double), (void **)&dr));
  BA_CHECK(ba_scratch(p, 2, (size_t)(24 * nobs + 2) * sizeof(double), (void **)&dJ));
  // [weights (nobs, padded to even) | 2 RED_BLOCKS partials | SUMSQ_JOBS RED_BLOCKS partials of the final sum | result]
  const int64_t wpad = (nobs + 1) & ~(int64_t)1;
  BA_CHECK(ba_scratch(p, 3, (size_t)(wpad + (2 + SUMSQ_JOBS) * RED_BLOCKS + 2) * sizeof(double), (void **)&dw));
  double *dpart = dw + wpad, *dmulti = dpart + 2 * RED_BLOCKS, *dout = dmulti + SUMSQ_JOBS * RED_BLOCKS;
  BA_HIP_CHECK(hipMemcpyAsync(dx, x, (size_t)nvar * sizeof(double), hipMemcpyHostToDevice, st));
  BA_CHECK(launch_residual_f64(p, dx, dr, st));
  BA_CHECK(launch_jac_coord_f64(p, dx, dJ, st));
  if (p->info_on()) BA_CHECK(launch_info_whiten(p, dr, dJ, dw, dpart, true, true, st));
  else BA_CHECK(launch_robust_scale(p, dr, dJ, dw, dpart, st));
  SumsqJobs jobs;
  jobs.add_sum(dpart, robust_blocks(nobs), dout, 0);
  BA_CHECK(launch_sumsq_multi(p, &jobs, dmulti, st));
  double sum = 0;
  if (weights && nobs > 0) BA_HIP_CHECK(hipMemcpyAsync(weights, dw, (size_t)nobs * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(&sum, dout, sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  if (cost) *cost = 0.5 * sum;
  return BA_OK;
}
