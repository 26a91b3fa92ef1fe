// The per-observation pass of the LM solve over r and J, k_obs_scale: the robust loss (ba_lm_set_loss) and the per-observation
// 2 x 2 information matrices (ba_lm_set_obs_info), and the entries that set, read and evaluate either on a handle.
//
// Robust loss: the LM loop linearises f(x) = 1/2 sum_i c^2 rho(|r_i|^2 / c^2) in the first-order (IRLS) form: r~_i = sqrt(w_i) r_i,
// J~_i = sqrt(w_i) J_i with w_i = rho'(z_i).  Information: observation i carries Lambda_i = L_i L_i' (L_i lower triangular,
// factored on the host) and the LM entries minimise 1/2 sum_i r_i' Lambda_i r_i (under a loss 1/2 sum_i c^2 rho(r_i' Lambda_i r_i /
// c^2)): with r^_i = L_i' r_i and J^_i = L_i' J_i that is the plain problem on r^ and J^, the loss's weights taken from |r^_i|^2.
// Either way the scaled J has the sparsity of J, so everything downstream of the Jacobian (the point and camera blocks, the
// Schur assembly, the factorisations, PCG, priors, the border, the covariance, the sharded path) runs unchanged.  k_obs_scale
// rewrites r and J in place right after the Jacobian kernel (and the mask), J read and written once, and leaves nothing per
// observation behind.
#include <algorithm>
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

constexpr int JH = JV / 2;  // 16-byte vectors of J per row

// One tile = OBS_TILE consecutive observations: thread t handles the residual pair (one 16-byte load and store) and the factors
// of observation t and puts the factors in LDS; then the tile's 12 OBS_TILE 16-byte vectors of J are streamed by the whole
// workgroup, vector k OBS_TILE + t by thread t -- contiguous 16-byte accesses across the lanes of a wave, the vector's
// observation (k OBS_TILE + t) / 12 read from LDS.  The loads of J are issued before the residual's arithmetic (12 vectors in
// flight per lane).  Workgroups stride over the tiles; the grid (obs_blocks) depends on nobs only, so the partial sums (cost
// sum c^2 rho(z) and |r~|^2, one each per workgroup, in a fixed tree; partial == null: none) do too.  One instantiation per
// loss: only its own rho stays live beside the 12 vectors of J.  416 bytes per observation without information.
// INFO: vector e of an observation holds columns 2 (e % 6), 2 (e % 6) + 1 of row e / 6, and
//   J^ row 0 = a row 0 + b row 1,   J^ row 1 = c row 1,   s = sqrt(w) (1 under the linear loss)
// so a vector of row 0 needs vector e + 6 of the same observation, which another lane holds (12 OBS_TILE + t has no two
// members 6 apart): the row-1 vectors of the tile go through LDS.  b == 0 (a diagonal Lambda) leaves row 1 out of row 0
// altogether: Lambda = I reproduces the pass without information bit for bit.  J == null (INFO only): the residual alone (the
// trial point of the LM loop).  whiten_r: r holds the plain residual (else r^ already: the accepted trial residual) -- the loss
// scaling applies either way.  440 bytes per observation.
// The two mixing statements of INFO (r^_x = l00 r_x + l10 r_y and J^ row 0) are kept from FMA contraction: they round as their
// plain restatement does (tests/helpers/info_ref.py; cancellation in a rank-one block makes a fused multiply-add miss the 1e-14 of
// the weights).  Everything else -- |r^|^2, rho, the sums -- is one set of statements for both modes, contracted as the compiler
// likes, so Lambda = I reproduces the pass without information bit for bit under every loss.
template <int KIND, bool INFO, bool WEIGHTS>
__global__ __launch_bounds__(OBS_TILE) void k_obs_scale(int64_t nobs, double c2, const double *__restrict__ L,
                                                        double2 *__restrict__ r, double2 *__restrict__ J,
                                                        double *__restrict__ wout, double *__restrict__ partial, int whiten_r) {
  // the factors of a tile's observations: sqrt(w), with INFO (a, b, c) = sqrt(w) (l00, l10, l11) beside the row-1 vectors of J
  // (24 KiB, declared in a branch that is discarded without INFO)
  __shared__ double sf[INFO ? 3 : 1][OBS_TILE];
  double2 *srow1 = nullptr;
  if constexpr (INFO) {
    __shared__ double2 row1[OBS_TILE * JH];
    srow1 = row1;
  }
  __shared__ double red[2][OBS_TILE / 64];
  const int t = threadIdx.x;
  const int64_t ntile = (nobs + OBS_TILE - 1) / OBS_TILE, nJ = nobs * JV;
  const bool jac = !INFO || J != nullptr;  // (uniform)
  double acc_c = 0, acc_r = 0;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t o = tile * OBS_TILE + t, j0 = tile * OBS_TILE * JV;
    double2 jv[JV];
    if (jac) {
#pragma unroll
      for (int k = 0; k < JV; k++) {
        const int64_t q = j0 + k * OBS_TILE + t;
        jv[k] = q < nJ ? J[q] : make_double2(0.0, 0.0);
      }
    }
    double a = 1.0, b = 0.0, c = 1.0;  // the factors: sqrt(w), with INFO (a, b, c)
    if (o < nobs) {
      double2 e = r[o];
      if constexpr (INFO) {
        a = L[3 * o], b = L[3 * o + 1], c = L[3 * o + 2];
        if (whiten_r) {
#pragma clang fp contract(off)
          e.x = a * e.x;
          if (b != 0.0) e.x += b * e.y;
          e.y = c * e.y;
        }
      }
      double w;
      acc_c += robust_rho(KIND, fma(e.x, e.x, e.y * e.y), c2, &w);  // (written out: contraction would pick either product)
      if (KIND != BA_LOSS_LINEAR) {
        const double s = sqrt(w);
        e.x *= s;
        e.y *= s;
        a *= s;
        if constexpr (INFO) b *= s, c *= s;
      }
      if (KIND != BA_LOSS_LINEAR || (INFO && whiten_r)) r[o] = e;
      acc_r += e.x * e.x + e.y * e.y;
      if (WEIGHTS) wout[o] = w;
    }
    if (jac) {
      sf[0][t] = a;
      if constexpr (INFO) {
        sf[1][t] = b;
        sf[2][t] = c;
#pragma unroll
        for (int k = 0; k < JV; k++) {
          const int v = k * OBS_TILE + t, e = v % JV;
          if (e >= JH) srow1[(v / JV) * JH + (e - JH)] = jv[k];
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < JV; k++) {
        const int v = k * OBS_TILE + t;
        const int64_t q = j0 + v;
        if (q < nJ) {
          const int ol = v / JV, e = v % JV;
          double2 out = jv[k];
          if (!INFO || e < JH) {
            const double fa = sf[0][ol];
            out.x *= fa;
            out.y *= fa;
            if constexpr (INFO) {
              const double fb = sf[1][ol];
              if (fb != 0.0) {
#pragma clang fp contract(off)
                const double2 p1 = srow1[ol * JH + e];
                out.x += fb * p1.x;
                out.y += fb * p1.y;
              }
            }
          } else if constexpr (INFO) {
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

struct ObsArgs {
  int64_t nobs;
  double c2;
  const double *L;
  double *r, *J, *w, *partial;
  int whiten_r;
};

template <int KIND, bool INFO, bool WEIGHTS>
int launch_one(const ObsArgs &a, hipStream_t st) {
  return BA_LAUNCH((k_obs_scale<KIND, INFO, WEIGHTS>), obs_blocks(a.nobs), OBS_TILE, 0, st, a.nobs, a.c2, a.L, (double2 *)a.r,
                   (double2 *)a.J, a.w, a.partial, a.whiten_r);
}

template <int KIND>
int launch_kind(bool info, const ObsArgs &a, hipStream_t st) {
  if (info) return a.w ? launch_one<KIND, true, true>(a, st) : launch_one<KIND, true, false>(a, st);
  return a.w ? launch_one<KIND, false, true>(a, st) : launch_one<KIND, false, false>(a, st);
}

}  // namespace

int obs_blocks(int64_t nobs) {
  const int64_t ntile = (nobs + OBS_TILE - 1) / OBS_TILE;
  return (int)(ntile < 1 ? 1 : (ntile > RED_BLOCKS ? RED_BLOCKS : ntile));
}

int launch_obs_scale(ba_problem *p, double *d_r, double *d_J, double *d_w, double *d_partial, bool residual_plain, bool with_loss,
                     hipStream_t st) {
  const int kind = with_loss ? p->loss : BA_LOSS_LINEAR;
  const bool info = p->info_on();
  // (partials that are asked for are always written: a launch of one workgroup at nobs = 0)
  if (!d_partial && ((!info && kind == BA_LOSS_LINEAR) || p->nobs <= 0)) return BA_OK;
  ProfScope ps(p, info ? PC_INFO : PC_ROBUST, st);
  const ObsArgs a = {p->nobs, p->loss_scale * p->loss_scale, info ? (const double *)p->d_info : nullptr, d_r, d_J, d_w, d_partial,
                     residual_plain ? 1 : 0};
  switch (kind) {
    case BA_LOSS_HUBER: return launch_kind<BA_LOSS_HUBER>(info, a, st);
    case BA_LOSS_SOFT_L1: return launch_kind<BA_LOSS_SOFT_L1>(info, a, st);
    case BA_LOSS_CAUCHY: return launch_kind<BA_LOSS_CAUCHY>(info, a, st);
    case BA_LOSS_ARCTAN: return launch_kind<BA_LOSS_ARCTAN>(info, a, st);
    default: return launch_kind<BA_LOSS_LINEAR>(info, a, st);
  }
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

// r and J at x, k_obs_scale with the weights written out, the cost partials summed by the fixed tree of the LM loop; with
// per-observation information on the handle (ba_lm_set_obs_info): w and f of r' Lambda r
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
  BA_CHECK(launch_obs_scale(p, dr, dJ, dw, dpart, true, true, st));
  SumsqJobs jobs;
  jobs.add_sum(dpart, obs_blocks(nobs), dout, 0);
  BA_CHECK(launch_sumsq_multi(p, &jobs, dmulti, st));
  double sum = 0;
  if (weights && nobs > 0) BA_HIP_CHECK(hipMemcpyAsync(weights, dw, (size_t)nobs * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(&sum, dout, sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  if (cost) *cost = 0.5 * sum;
  return BA_OK;
}

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
