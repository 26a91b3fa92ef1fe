// Gaussian priors of the LM solve (ba_lm_set_priors, include/ba_hip.h): the kernels that add the prior terms to the normal
// equations and evaluate their cost and model value, and the entries that set, read and evaluate the priors of a handle.
//
// f(x) = f_obs(x) + 1/2 sum_k d_k' Lambda_k d_k,  d_k = h_k(x) - mu_k,  h_k a point, a camera block or a camera centre
// c(r, t) = -R(r)' t.  With H_k = dh_k/dx a prior adds H_k' Lambda_k d_k to the gradient and H_k' Lambda_k H_k to the
// Gauss-Newton matrix, both inside ONE diagonal block (Hpp of its point, Hcc of its camera), so everything downstream of the
// blocks (point elimination, the Schur assembly and its tile pattern, the factorisations, PCG, the column scalings) runs
// unchanged.  One lane owns one prior and an index appears once per kind: plain read-modify-write, no atomics, and the
// kinds are launched one after the other on the stream, so a camera with a camera prior AND a centre prior is summed in a
// fixed order.  The values the controller needs (2 f_prior at x and at the trial point, the model term of a step) are written
// one per prior and summed by the fixed tree of launch_sumsq_multi (SumsqJobs::add_sum).
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

constexpr int PB = 256;  // priors per workgroup = threads per workgroup

// packed lower row-major 3 x 3 (l00 l10 l11 l20 l21 l22) times a 3-vector
__device__ __forceinline__ void sym3_mul(const double *__restrict__ l, const double e[3], double w[3]) {
  w[0] = l[0] * e[0] + l[1] * e[1] + l[3] * e[2];
  w[1] = l[1] * e[0] + l[2] * e[1] + l[4] * e[2];
  w[2] = l[3] * e[0] + l[4] * e[1] + l[5] * e[2];
}
__device__ __forceinline__ double sym3_quad(const double *__restrict__ l, const double e[3]) {
  double w[3];
  sym3_mul(l, e, w);
  return e[0] * w[0] + e[1] * w[1] + e[2] * w[2];
}
// packed lower row-major 9 x 9 (45): e' L e, streamed entry by entry (nothing of the block stays live)
__device__ __forceinline__ double sym9_quad(const double *__restrict__ l, const double e[9]) {
  double q = 0;
  int t = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
#pragma unroll
    for (int j = 0; j < i; j++) q += 2.0 * (l[t++] * e[i] * e[j]);
    q += l[t++] * e[i] * e[i];
  }
  return q;
}

#include "ba_prior_dev.h"  // centre_of

// ---- at a linearisation -------------------------------------------------------------------------------------------------
// point priors: H = I.  Hpp is stored xx xy xz yy yz zz, the prior's Lambda as packed lower row-major (xx xy yy xz yz zz).
// A fixed point keeps its cost (a constant of the solve) and adds nothing to its block and gradient: both stay exactly 0.
__global__ __launch_bounds__(PB) void k_prior_point_lin(int64_t n, const int *__restrict__ idx, const double *__restrict__ mu,
                                                        const double *__restrict__ info, const double *__restrict__ x,
                                                        const uint8_t *__restrict__ fix_pnt, double *__restrict__ Hpp,
                                                        double *__restrict__ gp, double *__restrict__ dlin,
                                                        double *__restrict__ cost) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t j = idx[q];
  const double *__restrict__ l = info + 6 * q;
  const double d[3] = {x[3 * j] - mu[3 * q], x[3 * j + 1] - mu[3 * q + 1], x[3 * j + 2] - mu[3 * q + 2]};
  double w[3];
  sym3_mul(l, d, w);
#pragma unroll
  for (int i = 0; i < 3; i++) dlin[3 * q + i] = d[i];
  cost[q] = d[0] * w[0] + d[1] * w[1] + d[2] * w[2];
  if (fix_pnt && fix_pnt[j]) return;
  double *__restrict__ h = Hpp + 6 * j;
  h[0] += l[0];
  h[1] += l[1];
  h[2] += l[3];
  h[3] += l[2];
  h[4] += l[4];
  h[5] += l[5];
#pragma unroll
  for (int i = 0; i < 3; i++) gp[3 * j + i] += w[i];
}

// camera priors: H = I with the columns of the camera's fixed components zeroed.  The 45 entries of Lambda are streamed once:
// each goes into Lambda d and, when neither of its components is fixed, into Hcc (same packing).
__global__ __launch_bounds__(PB) void k_prior_cam_lin(int64_t n, const int *__restrict__ idx, const double *__restrict__ mu,
                                                      const double *__restrict__ info, const double *__restrict__ xc,
                                                      const uint16_t *__restrict__ fix_cam, double *__restrict__ Hcc,
                                                      double *__restrict__ gc, double *__restrict__ dlin,
                                                      double *__restrict__ cost) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t c = idx[q];
  const unsigned fm = fix_cam ? fix_cam[c] : 0u;
  const double *__restrict__ l = info + 45 * q;
  double *__restrict__ h = Hcc + 45 * c;
  double d[9], w[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    d[i] = xc[9 * c + i] - mu[9 * q + i];
    dlin[9 * q + i] = d[i];
    w[i] = 0;
  }
  int t = 0;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j <= i; j++, t++) {
      const double v = l[t];
      w[i] += v * d[j];
      if (j < i) w[j] += v * d[i];
      if (!(((fm >> i) | (fm >> j)) & 1u)) h[t] += v;
    }
  double f = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    f += d[i] * w[i];
    if (!((fm >> i) & 1u)) gc[9 * c + i] += w[i];
  }
  cost[q] = f;
}

// centre priors: H = dc/d(r, t) (3 x 6, the columns of fixed components zeroed) is kept in Hlin for the model term of the
// steps solved at this linearisation; H' Lambda H goes into the leading 6 x 6 of the camera's block, H' Lambda d into gc[0..5]
__global__ __launch_bounds__(PB) void k_prior_ctr_lin(int64_t n, const int *__restrict__ idx, const double *__restrict__ mu,
                                                      const double *__restrict__ info, const double *__restrict__ xc,
                                                      const uint16_t *__restrict__ fix_cam, double *__restrict__ Hcc,
                                                      double *__restrict__ gc, double *__restrict__ dlin,
                                                      double *__restrict__ Hlin, double *__restrict__ cost) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t c = idx[q];
  const unsigned fm = fix_cam ? fix_cam[c] : 0u;
  const double *__restrict__ l = info + 6 * q;
  double ctr[3], H[18];
  centre_of<true>(xc + 9 * c, ctr, H);
  const double d[3] = {ctr[0] - mu[3 * q], ctr[1] - mu[3 * q + 1], ctr[2] - mu[3 * q + 2]};
  double w[3];
  sym3_mul(l, d, w);
  cost[q] = d[0] * w[0] + d[1] * w[1] + d[2] * w[2];
#pragma unroll
  for (int i = 0; i < 3; i++) dlin[3 * q + i] = d[i];
  double M[18];  // Lambda H
#pragma unroll
  for (int j = 0; j < 6; j++) {
    if ((fm >> j) & 1u) H[j] = H[6 + j] = H[12 + j] = 0.0;
    const double e[3] = {H[j], H[6 + j], H[12 + j]};
    double v[3];
    sym3_mul(l, e, v);
    M[j] = v[0];
    M[6 + j] = v[1];
    M[12 + j] = v[2];
  }
#pragma unroll
  for (int i = 0; i < 18; i++) Hlin[18 * q + i] = H[i];
  double *__restrict__ h = Hcc + 45 * c;
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++, t++) h[t] += (H[i] * M[j] + H[6 + i] * M[6 + j]) + H[12 + i] * M[12 + j];
    gc[9 * c + i] += (H[i] * w[0] + H[6 + i] * w[1]) + H[12 + i] * w[2];
  }
}

// ---- per trial step: the model term at the stored linearisation (delta != null) and the cost at xt (xt != null) -----------
__global__ __launch_bounds__(PB) void k_prior_point_step(int64_t n, const int *__restrict__ idx, const double *__restrict__ mu,
                                                         const double *__restrict__ info, const double *__restrict__ dlin,
                                                         const double *__restrict__ delta, const double *__restrict__ xt,
                                                         double *__restrict__ model, double *__restrict__ cost_t) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t j = idx[q];
  const double *__restrict__ l = info + 6 * q;
  if (delta) {
    const double e[3] = {delta[3 * j] + dlin[3 * q], delta[3 * j + 1] + dlin[3 * q + 1], delta[3 * j + 2] + dlin[3 * q + 2]};
    model[q] = sym3_quad(l, e);
  }
  if (xt) {
    const double e[3] = {xt[3 * j] - mu[3 * q], xt[3 * j + 1] - mu[3 * q + 1], xt[3 * j + 2] - mu[3 * q + 2]};
    cost_t[q] = sym3_quad(l, e);
  }
}

// (deltac / xtc: the camera part of delta / xt)
__global__ __launch_bounds__(PB) void k_prior_cam_step(int64_t n, const int *__restrict__ idx, const double *__restrict__ mu,
                                                       const double *__restrict__ info, const double *__restrict__ dlin,
                                                       const double *__restrict__ deltac, const double *__restrict__ xtc,
                                                       double *__restrict__ model, double *__restrict__ cost_t) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t c = idx[q];
  const double *__restrict__ l = info + 45 * q;
  double e[9];
  if (deltac) {
#pragma unroll
    for (int i = 0; i < 9; i++) e[i] = deltac[9 * c + i] + dlin[9 * q + i];
    model[q] = sym9_quad(l, e);
  }
  if (xtc) {
#pragma unroll
    for (int i = 0; i < 9; i++) e[i] = xtc[9 * c + i] - mu[9 * q + i];
    cost_t[q] = sym9_quad(l, e);
  }
}

__global__ __launch_bounds__(PB) void k_prior_ctr_step(int64_t n, const int *__restrict__ idx, const double *__restrict__ mu,
                                                       const double *__restrict__ info, const double *__restrict__ dlin,
                                                       const double *__restrict__ Hlin, const double *__restrict__ deltac,
                                                       const double *__restrict__ xtc, double *__restrict__ model,
                                                       double *__restrict__ cost_t) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t c = idx[q];
  const double *__restrict__ l = info + 6 * q;
  if (deltac) {
    const double *__restrict__ H = Hlin + 18 * q, *__restrict__ dc = deltac + 9 * c;
    double e[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      double v = dlin[3 * q + i];
#pragma unroll
      for (int j = 0; j < 6; j++) v += H[6 * i + j] * dc[j];
      e[i] = v;
    }
    model[q] = sym3_quad(l, e);
  }
  if (xtc) {
    double ctr[3];
    centre_of<false>(xtc + 9 * c, ctr, nullptr);
    const double e[3] = {ctr[0] - mu[3 * q], ctr[1] - mu[3 * q + 1], ctr[2] - mu[3 * q + 2]};
    cost_t[q] = sym3_quad(l, e);
  }
}

// ---- per linear step: the priors' share of the camera right-hand side ------------------------------------------------------
// launch_schur_rhs rebuilds rhs = W u - B' r from J and r (u = U^-1 gp carries the point priors, B' r is the observations' gc
// only), so H' Lambda d of the camera and centre priors is subtracted here, from d and H of the stored linearisation; opos:
// the camera's block row of S.  One prior, one block row; the two kinds one after the other on the stream.
__global__ __launch_bounds__(PB) void k_prior_cam_rhs(int64_t n, const int *__restrict__ idx, const double *__restrict__ info,
                                                      const double *__restrict__ dlin, const uint16_t *__restrict__ fix_cam,
                                                      const int *__restrict__ opos, double *__restrict__ rhs) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t c = idx[q];
  const unsigned fm = fix_cam ? fix_cam[c] : 0u;
  const double *__restrict__ l = info + 45 * q;
  double d[9], w[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    d[i] = dlin[9 * q + i];
    w[i] = 0;
  }
  int t = 0;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j <= i; j++, t++) {
      const double v = l[t];
      w[i] += v * d[j];
      if (j < i) w[j] += v * d[i];
    }
  double *__restrict__ out = rhs + 9 * (int64_t)(opos ? opos[c] : c);
#pragma unroll
  for (int i = 0; i < 9; i++)
    if (!((fm >> i) & 1u)) out[i] -= w[i];
}

// (Hlin: the columns of fixed components are zero already)
__global__ __launch_bounds__(PB) void k_prior_ctr_rhs(int64_t n, const int *__restrict__ idx, const double *__restrict__ info,
                                                      const double *__restrict__ dlin, const double *__restrict__ Hlin,
                                                      const int *__restrict__ opos, double *__restrict__ rhs) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= n) return;
  const int64_t c = idx[q];
  const double *__restrict__ H = Hlin + 18 * q;
  const double d[3] = {dlin[3 * q], dlin[3 * q + 1], dlin[3 * q + 2]};
  double w[3];
  sym3_mul(info + 6 * q, d, w);
  double *__restrict__ out = rhs + 9 * (int64_t)(opos ? opos[c] : c);
#pragma unroll
  for (int i = 0; i < 6; i++) out[i] -= (H[i] * w[0] + H[6 + i] * w[1]) + H[12 + i] * w[2];
}

}  // namespace

// the handle's priors to the device, once per change (ba_lm_set_priors marks them dirty), with the buffers the kernels write
int prior_upload(ba_problem *p) {
  if (!p->pri_dirty) return BA_OK;
  for (PriorSet &s : p->pri) {
    if (s.n == 0) continue;
    BA_CHECK(upload(s.idx, s.h_idx));
    BA_CHECK(upload(s.mu, s.h_mu));
    BA_CHECK(upload(s.info, s.h_info));
  }
  if (p->pri_on()) {
    BA_CHECK(p->pri_d.alloc(3 * p->pri[PRI_PNT].n + 9 * p->pri[PRI_CAM].n + 3 * p->pri[PRI_CTR].n));
    BA_CHECK(p->pri_H.alloc(18 * p->pri[PRI_CTR].n));
    BA_CHECK(p->pri_val.alloc(3 * p->pri_total()));
  }
  p->pri_dirty = false;
  return BA_OK;
}

int launch_prior_lin(ba_problem *p, const double *d_x, double *d_Hpp, double *d_gp, double *d_Hcc, double *d_gc, hipStream_t st) {
  if (!p->pri_on()) return BA_OK;
  ProfScope ps(p, PC_PRIOR, st);
  const PriorSet &pt = p->pri[PRI_PNT], &cm = p->pri[PRI_CAM], &ct = p->pri[PRI_CTR];
  const uint16_t *fc = p->fix_ncam > 0 ? (const uint16_t *)p->d_fix_cam : nullptr;
  const uint8_t *fp = p->fix_npnt > 0 ? (const uint8_t *)p->d_fix_pnt : nullptr;
  const double *xc = d_x + 3 * p->npnts;
  double *d = p->pri_d, *cost = p->pri_cost();
  BA_CHECK(BA_LAUNCH(k_prior_point_lin, grid_for(pt.n, PB), PB, 0, st, pt.n, pt.idx, pt.mu, pt.info, d_x, fp, d_Hpp, d_gp, d, cost));
  BA_CHECK(BA_LAUNCH(k_prior_cam_lin, grid_for(cm.n, PB), PB, 0, st, cm.n, cm.idx, cm.mu, cm.info, xc, fc, d_Hcc, d_gc, d + 3 * pt.n,
                     cost + pt.n));
  return BA_LAUNCH(k_prior_ctr_lin, grid_for(ct.n, PB), PB, 0, st, ct.n, ct.idx, ct.mu, ct.info, xc, fc, d_Hcc, d_gc,
                   d + 3 * pt.n + 9 * cm.n, p->pri_H, cost + pt.n + cm.n);
}

int launch_prior_rhs(ba_problem *p, double *d_rhs, const int *d_pos, hipStream_t st) {
  const PriorSet &pt = p->pri[PRI_PNT], &cm = p->pri[PRI_CAM], &ct = p->pri[PRI_CTR];
  if (cm.n + ct.n == 0) return BA_OK;
  ProfScope ps(p, PC_PRIOR, st);
  const uint16_t *fc = p->fix_ncam > 0 ? (const uint16_t *)p->d_fix_cam : nullptr;
  const double *d = p->pri_d;
  BA_CHECK(BA_LAUNCH(k_prior_cam_rhs, grid_for(cm.n, PB), PB, 0, st, cm.n, cm.idx, cm.info, d + 3 * pt.n, fc, d_pos, d_rhs));
  return BA_LAUNCH(k_prior_ctr_rhs, grid_for(ct.n, PB), PB, 0, st, ct.n, ct.idx, ct.info, d + 3 * pt.n + 9 * cm.n, p->pri_H, d_pos,
                   d_rhs);
}

int launch_prior_step(ba_problem *p, const double *d_delta, const double *d_xt, hipStream_t st) {
  if (!p->pri_on() || (!d_delta && !d_xt)) return BA_OK;
  ProfScope ps(p, PC_PRIOR, st);
  const PriorSet &pt = p->pri[PRI_PNT], &cm = p->pri[PRI_CAM], &ct = p->pri[PRI_CTR];
  const double *dc = d_delta ? d_delta + 3 * p->npnts : nullptr, *xc = d_xt ? d_xt + 3 * p->npnts : nullptr;
  const double *d = p->pri_d;
  double *model = p->pri_model(), *cost_t = p->pri_cost_trial();
  BA_CHECK(BA_LAUNCH(k_prior_point_step, grid_for(pt.n, PB), PB, 0, st, pt.n, pt.idx, pt.mu, pt.info, d, d_delta, d_xt, model, cost_t));
  BA_CHECK(BA_LAUNCH(k_prior_cam_step, grid_for(cm.n, PB), PB, 0, st, cm.n, cm.idx, cm.mu, cm.info, d + 3 * pt.n, dc, xc, model + pt.n,
                     cost_t + pt.n));
  return BA_LAUNCH(k_prior_ctr_step, grid_for(ct.n, PB), PB, 0, st, ct.n, ct.idx, ct.mu, ct.info, d + 3 * pt.n + 9 * cm.n, p->pri_H, dc, xc,
                   model + pt.n + cm.n, cost_t + pt.n + cm.n);
}

// one kind's lists checked and copied to the handle's staging (dim: entries of h_k, 3 or 9)
static int check_kind(const char *what, int dim, int64_t limit, int64_t n, const int64_t *idx1, const double *mu, const double *info,
                      PriorSet *out) {
  const int ninfo = dim * (dim + 1) / 2;
  if (n < 0 || (n > 0 && (!idx1 || !mu || !info))) {
    ba_set_error("ba_lm_set_priors: %s priors: negative count or null array", what);
    return BA_ERR_ARG;
  }
  std::vector<unsigned char> seen(n > 0 ? (size_t)limit : 0, 0);  // (nothing to allocate for a kind without priors)
  for (int64_t q = 0; q < n; q++) {
    const int64_t j = idx1[q];
    if (j < 1 || j > limit) {
      ba_set_error("ba_lm_set_priors: %s prior %lld has index %lld outside 1..%lld", what, (long long)(q + 1), (long long)j,
                   (long long)limit);
      return BA_ERR_ARG;
    }
    if (seen[(size_t)(j - 1)]) {
      ba_set_error("ba_lm_set_priors: index %lld appears twice among the %s priors", (long long)j, what);
      return BA_ERR_ARG;
    }
    seen[(size_t)(j - 1)] = 1;
    for (int i = 0; i < dim; i++)
      if (!std::isfinite(mu[dim * q + i])) {
        ba_set_error("ba_lm_set_priors: %s prior %lld has a mean that is not finite", what, (long long)(q + 1));
        return BA_ERR_ARG;
      }
    const double *l = info + (int64_t)ninfo * q;
    for (int i = 0; i < ninfo; i++)
      if (!std::isfinite(l[i])) {
        ba_set_error("ba_lm_set_priors: %s prior %lld has an information entry that is not finite", what, (long long)(q + 1));
        return BA_ERR_ARG;
      }
    for (int i = 0; i < dim; i++) {
      const double lii = l[i * (i + 1) / 2 + i];
      if (lii < 0) {
        ba_set_error("ba_lm_set_priors: %s prior %lld has the negative diagonal information entry %g", what, (long long)(q + 1), lii);
        return BA_ERR_ARG;
      }
      for (int j2 = 0; j2 < i; j2++) {
        const double lij = l[i * (i + 1) / 2 + j2], ljj = l[j2 * (j2 + 1) / 2 + j2];
        if (lij * lij > lii * ljj) {
          ba_set_error("ba_lm_set_priors: %s prior %lld: information entry (%d, %d) squared exceeds the product of its diagonal "
                       "entries (not positive semi-definite)", what, (long long)(q + 1), i + 1, j2 + 1);
          return BA_ERR_ARG;
        }
      }
    }
  }
  out->n = n;
  out->h_idx.resize((size_t)n);
  for (int64_t q = 0; q < n; q++) out->h_idx[(size_t)q] = (int)(idx1[q] - 1);
  out->h_mu.assign(mu, mu + (n > 0 ? dim * n : 0));
  out->h_info.assign(info, info + (n > 0 ? (int64_t)ninfo * n : 0));
  return BA_OK;
}

extern "C" int ba_lm_set_priors(ba_problem *p, int64_t n_pnt, const int64_t *pnt_idx1, const double *pnt_mu, const double *pnt_info,
                                int64_t n_cam, const int64_t *cam_idx1, const double *cam_mu, const double *cam_info, int64_t n_ctr,
                                const int64_t *ctr_idx1, const double *ctr_mu, const double *ctr_info) {
  if (!p) {
    ba_set_error("ba_lm_set_priors: null handle");
    return BA_ERR_ARG;
  }
  // (checked whole before the handle changes; no device call: uploaded when a step or solve runs)
  PriorSet next[PRI_KINDS];
  BA_CHECK(check_kind("point", 3, p->npnts, n_pnt, pnt_idx1, pnt_mu, pnt_info, &next[PRI_PNT]));
  BA_CHECK(check_kind("camera", 9, p->ncams, n_cam, cam_idx1, cam_mu, cam_info, &next[PRI_CAM]));
  BA_CHECK(check_kind("centre", 3, p->ncams, n_ctr, ctr_idx1, ctr_mu, ctr_info, &next[PRI_CTR]));
  for (int k = 0; k < PRI_KINDS; k++) {
    p->pri[k].n = next[k].n;
    p->pri[k].h_idx.swap(next[k].h_idx);
    p->pri[k].h_mu.swap(next[k].h_mu);
    p->pri[k].h_info.swap(next[k].h_info);
  }
  p->pri_version++;
  p->pri_dirty = p->pri_on();  // (a handle whose priors are cleared keeps its device buffers, unused)
  return BA_OK;
}

extern "C" int ba_lm_get_priors(const ba_problem *p, int64_t *n_pnt, int64_t *n_cam, int64_t *n_ctr) {
  if (!p) {
    ba_set_error("ba_lm_get_priors: null handle");
    return BA_ERR_ARG;
  }
  if (n_pnt) *n_pnt = p->pri[PRI_PNT].n;
  if (n_cam) *n_cam = p->pri[PRI_CAM].n;
  if (n_ctr) *n_ctr = p->pri[PRI_CTR].n;
  return BA_OK;
}

// d_k' Lambda_k d_k of every prior at x (k_prior_*_step's cost pass), summed by the fixed tree of the LM loop
extern "C" int ba_prior_eval(ba_problem *p, const double *x, double *cost, double *chi2_pnt, double *chi2_cam, double *chi2_ctr) {
  if (!p || !x) {
    ba_set_error("ba_prior_eval: null argument");
    return BA_ERR_ARG;
  }
  if (cost) *cost = 0.0;
  if (!p->pri_on()) return BA_OK;
  BA_HIP_CHECK(hipSetDevice(p->device));
  BA_CHECK(terms_upload(p));
  const int64_t nvar = 9 * p->ncams + 3 * p->npnts;
  hipStream_t st = p->stream;
  double *dx, *dsum;
  BA_CHECK(ba_scratch(p, 0, (size_t)(nvar + 1) * sizeof(double), (void **)&dx));
  BA_CHECK(ba_scratch(p, 3, (size_t)(SUMSQ_JOBS * RED_BLOCKS + 2) * sizeof(double), (void **)&dsum));
  double *dout = dsum + SUMSQ_JOBS * RED_BLOCKS;
  BA_HIP_CHECK(hipMemcpyAsync(dx, x, (size_t)nvar * sizeof(double), hipMemcpyHostToDevice, st));
  BA_CHECK(launch_prior_step(p, nullptr, dx, st));
  SumsqJobs jobs;
  jobs.add_sum(p->pri_cost_trial(), p->pri_total(), dout, 0);
  BA_CHECK(launch_sumsq_multi(p, &jobs, dsum, st));
  double sum = 0;
  const double *v = p->pri_cost_trial();
  double *outs[PRI_KINDS] = {chi2_pnt, chi2_cam, chi2_ctr};
  for (int k = 0; k < PRI_KINDS; k++) {
    if (outs[k] && p->pri[k].n > 0)
      BA_HIP_CHECK(hipMemcpyAsync(outs[k], v, (size_t)p->pri[k].n * sizeof(double), hipMemcpyDeviceToHost, st));
    v += p->pri[k].n;
  }
  BA_HIP_CHECK(hipMemcpyAsync(&sum, dout, sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  if (cost) *cost = 0.5 * sum;
  return BA_OK;
}
