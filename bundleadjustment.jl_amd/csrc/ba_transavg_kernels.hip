// Translation averaging over the view graph (ba_translation_loops, ba_average_translations; include/ba_hip.h, "translation
// averaging"): the kernels and the two device entries.  gfx950 only.  The host side of the graph -- the checks on
// the pair list, the CSR adjacency, the spanning forest -- is ba_view_graph.cpp; the scalar decisions of the Levenberg-Marquardt
// loop are ba_transavg_control.h.  Neither needs a device.
// k_transavg_prepare: one lane per pair, the direction normalised.
// k_translation_loops: ONE WAVE PER PAIR (a, b), the shape of k_rotation_loops.  The lanes stride over the shorter of the two
//   adjacency lists and bisect the other; a hit is a triangle: the distance of the pair's direction to the arc between the two
//   other directions, in registers.  The two counts are reduced across the wave as integers; one writer per output.
// k_transavg_linearise: one lane per pair: A_k (6), g_k (3), the cost term; on request the residual angle and rho'.
// k_transavg_camera: ONE WAVE PER CAMERA: the gradient and the 3 x 3 diagonal block of H gathered over the camera's list through
//   the fixed-order wave_sum; lane 0 adds lambda diag H and inverts the block.
// The conjugate gradient, per iteration four launches that never leave the device: k_transavg_matvec (one wave per camera: q = (H
//   + lambda diag H) p, and p_i . q_i), k_transavg_alpha (one workgroup: the dot product in camera order, alpha),
//   k_transavg_update (one lane per camera: x, r, z = M r, and r_i . z_i), k_transavg_beta (one workgroup: |r|_M, the stop flag,
//   beta, p <- z + beta p).  Once the flag is set every one of them returns at once.
// k_transavg_sum: one workgroup, the terms in a fixed order.  k_transavg_trial: c + x.
#include <algorithm>
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"  // robust_rho, wave_sum
#include "ba_transavg_control.h"
#include "ba_view_graph.h"

namespace {

#include "ba_refine_dev.h"    // wave_all_sum_int
#include "ba_transavg_dev.h"  // vectors and symmetric 3 x 3 matrices in scalars, the arc distance

constexpr int TA_BLK = 256, TA_WAVES = TA_BLK / 64;
constexpr int TA_CG_BATCH = 16;       // iterations between two looks at the stop flag
constexpr double TA_MIN_LENGTH = 1e-12;  // a direction, or a baseline, below it has no orientation
enum { TA_SC_RZ = 0, TA_SC_R0 = 1, TA_SC_ALPHA = 2, TA_SC_BOUND = 3, TA_SC_COUNT = 4 };  // the scalars of a solve
enum { TA_ST_DONE = 0, TA_ST_ITERATIONS = 1, TA_ST_COUNT = 2 };                          // done: 1 converged, 2 p'Hp <= 0

__global__ __launch_bounds__(TA_BLK) void k_transavg_prepare(int64_t n, const double *__restrict__ in, double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * TA_BLK + threadIdx.x;
  if (k >= n) return;
  double d[3];
  vec3_load(in + 3 * k, false, d);
  const double nn = vec3_norm(d);
  out[3 * k] = d[0] / nn, out[3 * k + 1] = d[1] / nn, out[3 * k + 2] = d[2] / nn;
}

// the view graph as the kernels read it: camera c's entries [ptr[c], ptr[c + 1]) sorted by neighbour, edge = 2 * pair +
// (0: c is the pair's first camera, 1: its second)
struct TransavgGraph {
  const int *ptr, *nbr, *edge;
};

__global__ __launch_bounds__(TA_BLK) void k_translation_loops(int npairs, const int *__restrict__ pa, const int *__restrict__ pb,
                                                              const uint8_t *__restrict__ used, TransavgGraph g, const double *__restrict__ dir,
                                                              double threshold, int *__restrict__ n_loops, int *__restrict__ support) {
  const int lane = (int)threadIdx.x & 63, k = (int)blockIdx.x * TA_WAVES + ((int)threadIdx.x >> 6);
  if (k >= npairs) return;
  int nl = 0, ns = 0;
  if (used[k]) {
    const int a = pa[k], b = pb[k];
    const int a0 = g.ptr[a], a1 = g.ptr[a + 1], b0 = g.ptr[b], b1 = g.ptr[b + 1];
    const bool swap = b1 - b0 < a1 - a0;  // stride over the shorter list
    const int s0 = swap ? b0 : a0, s1 = swap ? b1 : a1, o0 = swap ? a0 : b0, o1 = swap ? a1 : b1;
    double dk[3];
    vec3_load(dir + 3 * (int64_t)k, false, dk);
    for (int e = s0 + lane; e < s1; e += 64) {
      const int c = g.nbr[e];
      int lo = o0, hi = o1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.nbr[mid] < c) lo = mid + 1;
        else hi = mid;
      }
      if (lo < o1 && g.nbr[lo] == c) {
        const int ea = swap ? g.edge[lo] : g.edge[e], eb = swap ? g.edge[e] : g.edge[lo];  // c in a's list, c in b's list
        double d1[3], d2[3], dist;
        vec3_load(dir + 3 * (int64_t)(ea >> 1), (ea & 1) == 1, d1);  // a -> c: listed (c, a) points the other way
        vec3_load(dir + 3 * (int64_t)(eb >> 1), (eb & 1) == 0, d2);  // c -> b: listed (b, c) points the other way
        if (arc_distance(dk, d1, d2, &dist)) {
          nl += 1;
          ns += dist <= threshold ? 1 : 0;
        }
      }
    }
    nl = wave_all_sum_int(nl);
    ns = wave_all_sum_int(ns);
  }
  if (lane == 0) n_loops[k] = nl, support[k] = ns;
}

struct TransavgEdgeArgs {
  int npairs;
  const int *pa, *pb, *comp;     // per pair its cameras (0-based); per camera its component (-1: none)
  const uint8_t *finite, *kept;  // per pair
  const double *dir, *w;
  int loss;
  double c2;
};

// The linearisation of the pairs at the positions c.  A kept pair with u = c_b - c_a, |u| >= 1e-12: u^ = u / |u|, r = u^ - d,
// omega = w rho'(|r|^2 / c^2), A = (omega / |u|^2)(I - u^ u^'), g = (omega / |u|)(r - (u^ . r) u^), term = w c^2 rho / 2.  A kept
// pair with |u| < 1e-12: A = 0, g = 0, term = w c^2 rho(4 / c^2) / 2.  A pair that is not kept: zeros.  With residual != null:
// residual = the angle between u^ and d for a pair with a usable direction inside one component (NaN else, and for |u| <
// 1e-12), weight = rho' on a kept pair, else 0.
__global__ __launch_bounds__(TA_BLK) void k_transavg_linearise(TransavgEdgeArgs a, const double *__restrict__ c, double *__restrict__ A,
                                                               double *__restrict__ g, double *__restrict__ term,
                                                               double *__restrict__ residual, double *__restrict__ weight) {
  const int k = (int)blockIdx.x * TA_BLK + (int)threadIdx.x;
  if (k >= a.npairs) return;
  const int ca = a.pa[k], cb = a.pb[k];
  double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gk[3] = {0.0, 0.0, 0.0}, cost = 0.0, rw = 0.0;
  double th = __longlong_as_double(0x7ff8000000000000ll);
  const bool kept = a.kept[k] != 0, inside = a.finite[k] && a.comp[ca] >= 0 && a.comp[ca] == a.comp[cb];
  if (kept || inside) {
    double u[3], d[3];
    u[0] = c[3 * (int64_t)cb] - c[3 * (int64_t)ca], u[1] = c[3 * (int64_t)cb + 1] - c[3 * (int64_t)ca + 1];
    u[2] = c[3 * (int64_t)cb + 2] - c[3 * (int64_t)ca + 2];
    vec3_load(a.dir + 3 * (int64_t)k, false, d);
    const double nu = vec3_norm(u);
    if (nu >= TA_MIN_LENGTH) {
      double r[3];
      u[0] = u[0] / nu, u[1] = u[1] / nu, u[2] = u[2] / nu;
      r[0] = u[0] - d[0], r[1] = u[1] - d[1], r[2] = u[2] - d[2];
      if (inside) th = vec3_angle(u, d);
      if (kept) {
        const double wk = a.w[k], val = robust_rho(a.loss, vec3_dot(r, r), a.c2, &rw);
        const double om = wk * rw, h = vec3_dot(u, r), s1 = om / nu, s2 = om / (nu * nu);
        cost = 0.5 * (wk * val);
        gk[0] = s1 * (r[0] - h * u[0]), gk[1] = s1 * (r[1] - h * u[1]), gk[2] = s1 * (r[2] - h * u[2]);
        S[0] = s2 * (1.0 - u[0] * u[0]), S[1] = s2 * (-(u[0] * u[1])), S[2] = s2 * (-(u[0] * u[2]));
        S[3] = s2 * (1.0 - u[1] * u[1]), S[4] = s2 * (-(u[1] * u[2])), S[5] = s2 * (1.0 - u[2] * u[2]);
      }
    } else if (kept) {
      cost = 0.5 * (a.w[k] * robust_rho(a.loss, 4.0, a.c2, &rw));
    }
  }
#pragma unroll
  for (int e = 0; e < 6; e++) A[6 * (int64_t)k + e] = S[e];
  g[3 * (int64_t)k] = gk[0], g[3 * (int64_t)k + 1] = gk[1], g[3 * (int64_t)k + 2] = gk[2];
  term[k] = cost;
  if (residual) residual[k] = th, weight[k] = rw;
}

// out[0] <- the sum of n terms in a fixed order: strided partial sums per thread, the tree of a wave, the four waves in order
__device__ __forceinline__ double block_sum(int n, const double *__restrict__ term, double *part) {
  const int t = (int)threadIdx.x;
  double s = 0.0;
  for (int k = t; k < n; k += TA_BLK) s += term[k];
  s = wave_sum(s);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(TA_BLK) void k_transavg_sum(int n, const double *__restrict__ term, double *__restrict__ out) {
  __shared__ double part[TA_WAVES];
  const double s = block_sum(n, term, part);
  if (threadIdx.x == 0) out[0] = s;
}

struct TransavgSolveArgs {
  int ncams;
  TransavgGraph g;              // the kept pairs
  const uint8_t *fixed;         // per camera
  uint8_t *active;              // per camera: takes part in the solve
  double *gc, *dg, *Minv;       // per camera: gradient (3), lambda diag H (3), the preconditioner (6)
  double *x, *r, *z, *p, *q;    // per camera, 3 each
  double *part;                 // per camera: the term of the dot product under way
  double *sc;                   // TA_SC_*
  int *st;                      // TA_ST_*
};

// camera i: g_i = sum of -g_k where i is the pair's first camera and +g_k where it is its second; D_i = sum A_k; the block
// D_i + lambda diag D_i and its inverse.  A held camera, or one whose block is singular, takes no part: its delta is 0.
__global__ __launch_bounds__(TA_BLK) void k_transavg_camera(TransavgSolveArgs a, double lambda, const double *__restrict__ A,
                                                            const double *__restrict__ g) {
  const int lane = (int)threadIdx.x & 63, i = (int)blockIdx.x * TA_WAVES + ((int)threadIdx.x >> 6);
  if (i >= a.ncams) return;
  double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gi[3] = {0.0, 0.0, 0.0};
  const int e1 = a.g.ptr[i + 1];
  for (int e = a.g.ptr[i] + lane; e < e1; e += 64) {
    const int ed = a.g.edge[e];
    const int64_t m = ed >> 1;
    double gk[3];
    vec3_load(g + 3 * m, (ed & 1) == 0, gk);
    gi[0] += gk[0], gi[1] += gk[1], gi[2] += gk[2];
#pragma unroll
    for (int s = 0; s < 6; s++) D[s] += A[6 * m + s];
  }
  gi[0] = wave_sum(gi[0]), gi[1] = wave_sum(gi[1]), gi[2] = wave_sum(gi[2]);
#pragma unroll
  for (int s = 0; s < 6; s++) D[s] = wave_sum(D[s]);
  if (lane != 0) return;
  const double l0 = lambda * D[0], l1 = lambda * D[3], l2 = lambda * D[5];
  double V[6];
  D[0] = D[0] + l0, D[3] = D[3] + l1, D[5] = D[5] + l2;
  const bool ok = sym3_inverse(D, V) && !a.fixed[i];
  a.active[i] = ok ? 1 : 0;
  a.gc[3 * (int64_t)i] = gi[0], a.gc[3 * (int64_t)i + 1] = gi[1], a.gc[3 * (int64_t)i + 2] = gi[2];
  a.dg[3 * (int64_t)i] = l0, a.dg[3 * (int64_t)i + 1] = l1, a.dg[3 * (int64_t)i + 2] = l2;
#pragma unroll
  for (int s = 0; s < 6; s++) a.Minv[6 * (int64_t)i + s] = ok ? V[s] : 0.0;
}

// z_i <- M_i r_i, and r_i . z_i
__device__ __forceinline__ double precondition(const TransavgSolveArgs &a, int64_t i, const double r[3]) {
  double V[6], z[3];
#pragma unroll
  for (int s = 0; s < 6; s++) V[s] = a.Minv[6 * i + s];
  sym3_mul(V, r, z);
  a.z[3 * i] = z[0], a.z[3 * i + 1] = z[1], a.z[3 * i + 2] = z[2];
  return vec3_dot(r, z);
}

// the start of a solve: x = 0, r = -g (0 where the camera takes no part), z = M r, p = z
__global__ __launch_bounds__(TA_BLK) void k_transavg_cg_init(TransavgSolveArgs a) {
  const int64_t i = (int64_t)blockIdx.x * TA_BLK + threadIdx.x;
  if (i >= a.ncams) return;
  const bool on = a.active[i] != 0;
  double r[3];
  r[0] = on ? -a.gc[3 * i] : 0.0, r[1] = on ? -a.gc[3 * i + 1] : 0.0, r[2] = on ? -a.gc[3 * i + 2] : 0.0;
  a.x[3 * i] = 0.0, a.x[3 * i + 1] = 0.0, a.x[3 * i + 2] = 0.0;
  a.r[3 * i] = r[0], a.r[3 * i + 1] = r[1], a.r[3 * i + 2] = r[2];
  a.part[i] = precondition(a, i, r);
  a.p[3 * i] = a.z[3 * i], a.p[3 * i + 1] = a.z[3 * i + 1], a.p[3 * i + 2] = a.z[3 * i + 2];
}

// |r0|_M and the bound cg_tol |r0|_M; a zero (or NaN) gradient ends the solve before its first iteration
__global__ __launch_bounds__(TA_BLK) void k_transavg_cg_start(TransavgSolveArgs a, double cg_tol) {
  __shared__ double part[TA_WAVES];
  const double rz = block_sum(a.ncams, a.part, part);
  if (threadIdx.x != 0) return;
  const double r0 = sqrt(rz);
  a.sc[TA_SC_RZ] = rz, a.sc[TA_SC_R0] = r0, a.sc[TA_SC_ALPHA] = 0.0, a.sc[TA_SC_BOUND] = cg_tol * r0;
  a.st[TA_ST_DONE] = r0 > 0.0 ? 0 : 1, a.st[TA_ST_ITERATIONS] = 0;
}

// q_i = sum over the camera's kept pairs of A_k (p_i - p_j) + lambda diag D_i p_i, and p_i . q_i
__global__ __launch_bounds__(TA_BLK) void k_transavg_matvec(TransavgSolveArgs a, const double *__restrict__ A) {
  const int lane = (int)threadIdx.x & 63, i = (int)blockIdx.x * TA_WAVES + ((int)threadIdx.x >> 6);
  if (i >= a.ncams || a.st[TA_ST_DONE]) return;
  double y[3] = {0.0, 0.0, 0.0}, pi[3];
  vec3_load(a.p + 3 * (int64_t)i, false, pi);
  if (a.active[i]) {
    const int e1 = a.g.ptr[i + 1];
    for (int e = a.g.ptr[i] + lane; e < e1; e += 64) {
      const int64_t j = a.g.nbr[e], m = a.g.edge[e] >> 1;
      double S[6], d[3], t[3];
#pragma unroll
      for (int s = 0; s < 6; s++) S[s] = A[6 * m + s];
      d[0] = pi[0] - a.p[3 * j], d[1] = pi[1] - a.p[3 * j + 1], d[2] = pi[2] - a.p[3 * j + 2];
      sym3_mul(S, d, t);
      y[0] += t[0], y[1] += t[1], y[2] += t[2];
    }
    y[0] = wave_sum(y[0]), y[1] = wave_sum(y[1]), y[2] = wave_sum(y[2]);
    y[0] = y[0] + a.dg[3 * (int64_t)i] * pi[0], y[1] = y[1] + a.dg[3 * (int64_t)i + 1] * pi[1], y[2] = y[2] + a.dg[3 * (int64_t)i + 2] * pi[2];
  }
  if (lane != 0) return;
  a.q[3 * (int64_t)i] = y[0], a.q[3 * (int64_t)i + 1] = y[1], a.q[3 * (int64_t)i + 2] = y[2];
  a.part[i] = vec3_dot(pi, y);
}

// alpha = r'z / p'q; p'q <= 0 (or NaN) ends the solve where it stands
__global__ __launch_bounds__(TA_BLK) void k_transavg_alpha(TransavgSolveArgs a) {
  __shared__ double part[TA_WAVES];
  if (a.st[TA_ST_DONE]) return;
  const double pq = block_sum(a.ncams, a.part, part);
  if (threadIdx.x != 0) return;
  if (pq > 0.0) a.sc[TA_SC_ALPHA] = a.sc[TA_SC_RZ] / pq;
  else a.st[TA_ST_DONE] = 2;
}

// x += alpha p, r -= alpha q, z = M r, and r_i . z_i
__global__ __launch_bounds__(TA_BLK) void k_transavg_update(TransavgSolveArgs a) {
  const int64_t i = (int64_t)blockIdx.x * TA_BLK + threadIdx.x;
  if (i >= a.ncams || a.st[TA_ST_DONE]) return;
  const double al = a.sc[TA_SC_ALPHA];
  double r[3];
  a.x[3 * i] = a.x[3 * i] + al * a.p[3 * i], a.x[3 * i + 1] = a.x[3 * i + 1] + al * a.p[3 * i + 1];
  a.x[3 * i + 2] = a.x[3 * i + 2] + al * a.p[3 * i + 2];
  r[0] = a.r[3 * i] - al * a.q[3 * i], r[1] = a.r[3 * i + 1] - al * a.q[3 * i + 1], r[2] = a.r[3 * i + 2] - al * a.q[3 * i + 2];
  a.r[3 * i] = r[0], a.r[3 * i + 1] = r[1], a.r[3 * i + 2] = r[2];
  a.part[i] = precondition(a, i, r);
}

// |r|_M = sqrt(r'z): at or below the bound (or NaN) the solve is done, x holding this iteration's step; else beta = r'z / the
// last r'z and p <- z + beta p
__global__ __launch_bounds__(TA_BLK) void k_transavg_beta(TransavgSolveArgs a) {
  __shared__ double part[TA_WAVES];
  if (a.st[TA_ST_DONE]) return;
  const double rzn = block_sum(a.ncams, a.part, part);
  const double rz = a.sc[TA_SC_RZ], bound = a.sc[TA_SC_BOUND];
  const bool more = sqrt(rzn) > bound;
  __syncthreads();  // (every thread has read the scalars that thread 0 writes next)
  if (threadIdx.x == 0) {
    a.st[TA_ST_ITERATIONS] = a.st[TA_ST_ITERATIONS] + 1;
    a.sc[TA_SC_RZ] = rzn;
    if (!more) a.st[TA_ST_DONE] = 1;
  }
  if (!more) return;
  const double beta = rzn / rz;
  for (int64_t e = threadIdx.x; e < 3 * (int64_t)a.ncams; e += TA_BLK) a.p[e] = a.z[e] + beta * a.p[e];
}

__global__ __launch_bounds__(TA_BLK) void k_transavg_trial(int64_t n, const double *__restrict__ c, const double *__restrict__ x,
                                                           double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * TA_BLK + threadIdx.x;
  if (e < n) out[e] = c[e] + x[e];
}

// what both entries check and upload: the pairs (0-based), "the direction is usable" (finite, norm >= 1e-12), used = the
// caller's (or all) and usable
struct TransavgInput {
  std::vector<int> pa, pb;
  std::vector<uint8_t> finite, used;
};

int transavg_input(const char *who, ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *dir,
                   const uint8_t *used, TransavgInput *in) {
  if (!p || (npairs > 0 && !dir)) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  if (view_graph_check(who, p->ncams, npairs, pair_a1, pair_b1)) return BA_ERR_ARG;
  const size_t n = (size_t)npairs;
  in->pa.resize(n), in->pb.resize(n), in->finite.resize(n), in->used.resize(n);
  for (size_t k = 0; k < n; k++) {
    const double x = dir[3 * k], y = dir[3 * k + 1], z = dir[3 * k + 2];
    in->pa[k] = (int)pair_a1[k] - 1, in->pb[k] = (int)pair_b1[k] - 1;
    in->finite[k] = std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && std::sqrt((x * x + y * y) + z * z) >= TA_MIN_LENGTH;
    in->used[k] = in->finite[k] && (!used || used[k]);
  }
  return BA_OK;
}

// the pairs, their flags and their normalised directions on the device
int transavg_upload(ba_problem *p, const TransavgInput &in, const double *dir, hipStream_t st) {
  TransavgWork &w = p->transavg;
  const int64_t n = (int64_t)in.pa.size();
  BA_CHECK(put(w.pa, in.pa, st));
  BA_CHECK(put(w.pb, in.pb, st));
  BA_CHECK(put(w.used, in.used, st));
  BA_CHECK(grow(w.dir_in, 3 * n));
  BA_CHECK(grow(w.dir, 3 * n));
  if (n > 0) BA_HIP_CHECK(hipMemcpyAsync((double *)w.dir_in, dir, (size_t)(3 * n) * sizeof(double), hipMemcpyHostToDevice, st));
  return BA_LAUNCH(k_transavg_prepare, grid_for(n, TA_BLK), TA_BLK, 0, st, n, w.dir_in, w.dir);
}

// the CSR adjacency of the pairs with mask != 0 on the device
int transavg_graph(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *mask, TransavgGraph *g,
                   hipStream_t st) {
  TransavgWork &w = p->transavg;
  std::vector<int> ptr, nbr, edge;
  view_graph_csr(p->ncams, npairs, pair_a1, pair_b1, mask, &ptr, &nbr, &edge);
  BA_CHECK(put(w.adj_ptr, ptr, st));
  BA_CHECK(put(w.adj_nbr, nbr, st));
  BA_CHECK(put(w.adj_edge, edge, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));  // (the host vectors end here)
  g->ptr = w.adj_ptr, g->nbr = w.adj_nbr, g->edge = w.adj_edge;
  return BA_OK;
}

// the loop counts of the uploaded pairs -> host
int transavg_loops(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const TransavgInput &in, double threshold,
                   int32_t *n_loops, int32_t *support, hipStream_t st) {
  TransavgWork &w = p->transavg;
  TransavgGraph g;
  BA_CHECK(transavg_graph(p, npairs, pair_a1, pair_b1, in.used.data(), &g, st));
  BA_CHECK(grow(w.n_loops, npairs));
  BA_CHECK(grow(w.support, npairs));
  {
    ProfScope ps(p, PC_TRANSAVG, st);
    BA_CHECK(BA_LAUNCH(k_translation_loops, grid_for(npairs, TA_WAVES), TA_BLK, 0, st, (int)npairs, w.pa, w.pb, w.used, g, w.dir, threshold,
                       w.n_loops, w.support));
  }
  BA_HIP_CHECK(hipMemcpyAsync(n_loops, w.n_loops, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(support, w.support, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

int transavg_opts_check(const char *who, const ba_transavg_opts *in, ba_transavg_opts *o) {
  if (!in) {
    ba_set_error("%s: null options", who);
    return BA_ERR_ARG;
  }
  *o = *in;
  if (o->loss < BA_LOSS_LINEAR || o->loss > BA_LOSS_ARCTAN) {
    ba_set_error("%s: loss must be one of BA_LOSS_*, got %d", who, o->loss);
    return BA_ERR_ARG;
  }
  if (o->loss != BA_LOSS_LINEAR && !(std::isfinite(o->f_scale) && o->f_scale > 0)) {
    ba_set_error("%s: f_scale (chordal units) must be finite and > 0 under a loss that is not linear, got %g", who, o->f_scale);
    return BA_ERR_ARG;
  }
  if (o->loss == BA_LOSS_LINEAR) o->f_scale = 1.0;
  if (o->loops) {
    if (!(std::isfinite(o->loop_threshold) && o->loop_threshold > 0)) {
      ba_set_error("%s: loop_threshold (radians) must be finite and > 0, got %g", who, o->loop_threshold);
      return BA_ERR_ARG;
    }
    if (!(o->min_ratio >= 0 && o->min_ratio <= 1)) {
      ba_set_error("%s: min_ratio must lie in [0, 1] (0: off), got %g", who, o->min_ratio);
      return BA_ERR_ARG;
    }
    if (o->min_support <= 0) o->min_support = 1;
  }
  if (o->max_iterations <= 0) o->max_iterations = 50;
  if (o->max_iterations > 100000) {
    ba_set_error("%s: max_iterations must be <= 100000, got %d", who, o->max_iterations);
    return BA_ERR_ARG;
  }
  if (o->max_cg <= 0) o->max_cg = 500;
  if (o->max_cg > 100000) {
    ba_set_error("%s: max_cg must be <= 100000, got %d", who, o->max_cg);
    return BA_ERR_ARG;
  }
  if (!std::isfinite(o->ftol) || !std::isfinite(o->cg_tol) || !std::isfinite(o->lambda0)) {
    ba_set_error("%s: ftol, cg_tol and lambda0 must be finite (<= 0: the default), got %g, %g, %g", who, o->ftol, o->cg_tol, o->lambda0);
    return BA_ERR_ARG;
  }
  if (o->ftol <= 0) o->ftol = 1e-10;
  if (o->cg_tol <= 0) o->cg_tol = 1e-6;
  if (o->lambda0 <= 0) o->lambda0 = 1e-3;
  return BA_OK;
}

// One solve of (H + lambda diag H) delta = -g at the linearisation (A, g): the result is w.x; the iterations are added to *total
int transavg_solve(ba_problem *p, const TransavgSolveArgs &sa, const double *A, const double *g, double lambda, const ba_transavg_opts &o,
                   int *iterations, hipStream_t st) {
  const int ncams = sa.ncams;
  BA_CHECK(BA_LAUNCH(k_transavg_camera, grid_for(ncams, TA_WAVES), TA_BLK, 0, st, sa, lambda, A, g));
  BA_CHECK(BA_LAUNCH(k_transavg_cg_init, grid_for(ncams, TA_BLK), TA_BLK, 0, st, sa));
  BA_CHECK(BA_LAUNCH(k_transavg_cg_start, 1, TA_BLK, 0, st, sa, o.cg_tol));
  int state[TA_ST_COUNT] = {0, 0};
  for (int done = 0; done < o.max_cg && !state[TA_ST_DONE];) {
    const int batch = std::min(TA_CG_BATCH, o.max_cg - done);
    for (int s = 0; s < batch; s++) {
      BA_CHECK(BA_LAUNCH(k_transavg_matvec, grid_for(ncams, TA_WAVES), TA_BLK, 0, st, sa, A));
      BA_CHECK(BA_LAUNCH(k_transavg_alpha, 1, TA_BLK, 0, st, sa));
      BA_CHECK(BA_LAUNCH(k_transavg_update, grid_for(ncams, TA_BLK), TA_BLK, 0, st, sa));
      BA_CHECK(BA_LAUNCH(k_transavg_beta, 1, TA_BLK, 0, st, sa));
    }
    BA_HIP_CHECK(hipMemcpyAsync(state, sa.st, sizeof(state), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    done += batch;
  }
  *iterations = state[TA_ST_ITERATIONS];
  return BA_OK;
}

}  // namespace

extern "C" int ba_transavg_lm_decide(double F, double F_trial, double lambda, int iteration, int max_iterations, double ftol,
                                     double *lambda_next, int *stop) {
  const TransavgDecision d = transavg_lm_decide(F, F_trial, lambda, iteration, max_iterations, ftol);
  if (lambda_next) *lambda_next = d.lambda;
  if (stop) *stop = d.stop;
  return d.accepted;
}

extern "C" int ba_translation_loops(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *dir,
                                    const uint8_t *used, double threshold, int32_t *n_loops, int32_t *support) {
  const char *who = "ba_translation_loops";
  if (!(std::isfinite(threshold) && threshold > 0)) {
    ba_set_error("%s: threshold (radians) must be finite and > 0, got %g", who, threshold);
    return BA_ERR_ARG;
  }
  TransavgInput in;
  BA_CHECK(transavg_input(who, p, npairs, pair_a1, pair_b1, dir, used, &in));
  if (npairs > 0 && (!n_loops || !support)) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  if (npairs == 0) return BA_OK;
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  BA_CHECK(transavg_upload(p, in, dir, st));
  return transavg_loops(p, npairs, pair_a1, pair_b1, in, threshold, n_loops, support, st);
}

extern "C" int ba_average_translations(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *dir,
                                       const double *weights, const uint8_t *used, const double *c0, const uint8_t *fixed,
                                       const ba_transavg_opts *opts, double *c, uint8_t *status, int32_t *component, uint8_t *kept,
                                       int32_t *n_loops, int32_t *support, double *residual, double *edge_weight, int32_t *iterations,
                                       int32_t *cg_iterations, double *trace, double *cost, int64_t *counts) {
  const char *who = "ba_average_translations";
  ba_transavg_opts o;
  BA_CHECK(transavg_opts_check(who, opts, &o));
  TransavgInput in;
  BA_CHECK(transavg_input(who, p, npairs, pair_a1, pair_b1, dir, used, &in));
  const int64_t ncams = p->ncams;
  const size_t nc = (size_t)ncams, np = (size_t)npairs;
  if ((ncams > 0 && (!c || !status || !component)) || (npairs > 0 && (!kept || !residual || !edge_weight)) || !iterations || !cg_iterations) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  for (size_t k = 0; weights && k < np; k++)
    if (!std::isfinite(weights[k]) || weights[k] < 0) {
      ba_set_error("%s: weights[%lld] = %g: a weight is finite and >= 0", who, (long long)k, weights[k]);
      return BA_ERR_ARG;
    }
  bool any_fixed = false;
  for (size_t i = 0; fixed && i < nc; i++) any_fixed = any_fixed || fixed[i];
  if (any_fixed && !c0) {
    ba_set_error("%s: fixed cameras are held at c0, which is null", who);
    return BA_ERR_ARG;
  }
  if (c0) {
    std::vector<uint8_t> touched(nc, 0);
    for (size_t k = 0; k < np; k++)
      if (in.used[k]) touched[(size_t)in.pa[k]] = touched[(size_t)in.pb[k]] = 1;
    for (size_t i = 0; i < nc; i++)
      if (touched[i] && !(std::isfinite(c0[3 * i]) && std::isfinite(c0[3 * i + 1]) && std::isfinite(c0[3 * i + 2]))) {
        ba_set_error("%s: c0 of camera %lld, which has a used pair, is not finite", who, (long long)i + 1);
        return BA_ERR_ARG;
      }
  }
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  TransavgWork &w = p->transavg;
  BA_CHECK(transavg_upload(p, in, dir, st));

  // the loop filter: a pair with checked triangles, too few of which close, is dropped
  std::vector<uint8_t> keep(in.used);
  std::vector<int32_t> nl, sup;
  if (o.loops && npairs > 0) {
    nl.resize(np), sup.resize(np);
    BA_CHECK(transavg_loops(p, npairs, pair_a1, pair_b1, in, o.loop_threshold, nl.data(), sup.data(), st));
    for (size_t k = 0; k < np; k++)
      if (keep[k] && nl[k] > 0 && (sup[k] < o.min_support || (double)sup[k] < o.min_ratio * (double)nl[k])) keep[k] = 0;
  }
  for (size_t k = 0; k < np; k++) {
    kept[k] = keep[k];
    if (n_loops) n_loops[k] = o.loops ? nl[k] : 0;
    if (support) support[k] = o.loops ? sup[k] : 0;
  }

  // the forest of the kept pairs: components, roots, and the start where c0 gives none
  ViewForest f;
  view_graph_forest(ncams, npairs, pair_a1, pair_b1, keep.data(), o.loops ? sup.data() : nullptr, weights, fixed, &f);
  std::vector<double> cs(3 * nc, 0.0);  // (a camera outside the graph: 0, never read)
  if (c0) {
    for (size_t i = 0; i < nc; i++)
      if (f.component[i] >= 0) cs[3 * i] = c0[3 * i], cs[3 * i + 1] = c0[3 * i + 1], cs[3 * i + 2] = c0[3 * i + 2];
  } else {
    std::vector<double> d(3 * np);
    if (npairs > 0) BA_HIP_CHECK(hipMemcpyAsync(d.data(), w.dir, 3 * np * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    for (int i : f.order) {  // child = parent +- d along the forest, parents first: every tree baseline has length 1
      const int64_t k = f.parent_pair[(size_t)i];
      if (k < 0) continue;
      const bool forward = in.pb[(size_t)k] == i;  // listed (parent, child)
      const int par = forward ? in.pa[(size_t)k] : in.pb[(size_t)k];
      for (int e = 0; e < 3; e++)
        cs[3 * (size_t)i + e] = forward ? cs[3 * (size_t)par + e] + d[3 * (size_t)k + e] : cs[3 * (size_t)par + e] - d[3 * (size_t)k + e];
    }
  }

  // per camera: held or not, the component; per pair: kept, usable, weight
  std::vector<uint8_t> fx(nc, 0), comp_fixed(f.roots.size(), 0);
  for (size_t i = 0; i < nc; i++)
    if (fixed && fixed[i] && f.component[i] >= 0) fx[i] = 1, comp_fixed[(size_t)f.component[i]] = 1;
  std::vector<double> wt(np, 1.0);
  for (size_t k = 0; weights && k < np; k++) wt[k] = weights[k];
  BA_CHECK(put(w.fixed, fx, st));
  BA_CHECK(put(w.comp, f.component, st));
  BA_CHECK(put(w.kept, keep, st));
  BA_CHECK(put(w.finite, in.finite, st));
  BA_CHECK(put(w.weight, wt, st));
  BA_CHECK(put(w.c[0], cs, st));
  BA_CHECK(grow(w.c[1], 3 * ncams));
  for (int s = 0; s < 2; s++) {
    BA_CHECK(grow(w.A[s], 6 * npairs));
    BA_CHECK(grow(w.g[s], 3 * npairs));
    BA_CHECK(grow(w.term[s], npairs));
  }
  BA_CHECK(grow(w.residual, npairs));
  BA_CHECK(grow(w.edge_weight, npairs));
  BA_CHECK(grow(w.active, ncams));
  BA_CHECK(grow(w.gc, 3 * ncams));
  BA_CHECK(grow(w.dg, 3 * ncams));
  BA_CHECK(grow(w.Minv, 6 * ncams));
  for (GrowBuf<double> *b : {&w.x, &w.r, &w.z, &w.p, &w.q}) BA_CHECK(grow(*b, 3 * ncams));
  BA_CHECK(grow(w.part, ncams));
  BA_CHECK(grow(w.sc, TA_SC_COUNT));
  BA_CHECK(grow(w.st, TA_ST_COUNT));
  BA_CHECK(grow(w.cost, 3));
  TransavgGraph g;
  BA_CHECK(transavg_graph(p, npairs, pair_a1, pair_b1, keep.data(), &g, st));  // (synchronises: the host vectors above end here too)

  const double c2 = o.f_scale * o.f_scale;
  TransavgEdgeArgs ea{(int)npairs, w.pa, w.pb, w.comp, w.finite, w.kept, w.dir, w.weight, o.loss, c2};
  TransavgSolveArgs sa{(int)ncams, g, w.fixed, w.active, w.gc, w.dg, w.Minv, w.x, w.r, w.z, w.p, w.q, w.part, w.sc, w.st};
  int64_t nkept = 0;
  for (size_t k = 0; k < np; k++) nkept += keep[k];
  double F = 0.0, F0 = 0.0, lambda = o.lambda0;
  int cur = 0, its = 0, cg_total = 0;
  std::vector<double> ch(3 * nc, 0.0);
  {
    ProfScope ps(p, PC_TRANSAVG, st);
    BA_CHECK(BA_LAUNCH(k_transavg_linearise, grid_for(npairs, TA_BLK), TA_BLK, 0, st, ea, w.c[0], w.A[0], w.g[0], w.term[0], (double *)nullptr,
                       (double *)nullptr));
    BA_CHECK(BA_LAUNCH(k_transavg_sum, 1, TA_BLK, 0, st, (int)npairs, w.term[0], w.cost));
    BA_HIP_CHECK(hipMemcpyAsync(&F, w.cost, sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    F0 = F;
    while (nkept > 0) {
      int cg = 0;
      double Ft = 0.0;
      its++;
      BA_CHECK(transavg_solve(p, sa, w.A[cur], w.g[cur], lambda, o, &cg, st));
      BA_CHECK(BA_LAUNCH(k_transavg_trial, grid_for(3 * ncams, TA_BLK), TA_BLK, 0, st, 3 * ncams, w.c[cur], w.x, w.c[cur ^ 1]));
      BA_CHECK(BA_LAUNCH(k_transavg_linearise, grid_for(npairs, TA_BLK), TA_BLK, 0, st, ea, w.c[cur ^ 1], w.A[cur ^ 1], w.g[cur ^ 1],
                         w.term[cur ^ 1], (double *)nullptr, (double *)nullptr));
      BA_CHECK(BA_LAUNCH(k_transavg_sum, 1, TA_BLK, 0, st, (int)npairs, w.term[cur ^ 1], (double *)w.cost + 2));
      BA_HIP_CHECK(hipMemcpyAsync(&Ft, (double *)w.cost + 2, sizeof(double), hipMemcpyDeviceToHost, st));
      BA_HIP_CHECK(hipStreamSynchronize(st));
      const TransavgDecision d = transavg_lm_decide(F, Ft, lambda, its, o.max_iterations, o.ftol);
      if (trace) trace[4 * (its - 1)] = Ft, trace[4 * (its - 1) + 1] = lambda, trace[4 * (its - 1) + 2] = cg, trace[4 * (its - 1) + 3] = d.accepted;
      cg_total += cg;
      lambda = d.lambda;
      if (d.accepted) cur ^= 1, F = Ft;
      if (d.stop) break;
    }
    // the gauge, on the host: a component without a held camera is moved so that its root is back at its start and scaled
    // about the root so that the mean length of its kept baselines (summed in pair order) is that of the start
    if (ncams > 0) BA_HIP_CHECK(hipMemcpyAsync(ch.data(), w.c[cur], 3 * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    const size_t ng = f.roots.size();
    std::vector<double> len0(ng, 0.0), len1(ng, 0.0);
    auto baseline = [&](const std::vector<double> &v, size_t k) {
      const size_t a = (size_t)in.pa[k], b = (size_t)in.pb[k];
      const double x = v[3 * b] - v[3 * a], y = v[3 * b + 1] - v[3 * a + 1], z = v[3 * b + 2] - v[3 * a + 2];
      return std::sqrt((x * x + y * y) + z * z);
    };
    for (size_t k = 0; k < np; k++)
      if (keep[k]) len0[(size_t)f.component[(size_t)in.pa[k]]] += baseline(cs, k), len1[(size_t)f.component[(size_t)in.pa[k]]] += baseline(ch, k);
    std::vector<double> out(ch);
    for (size_t i = 0; i < nc; i++) {
      const int gi = f.component[i];
      if (gi < 0 || comp_fixed[(size_t)gi]) continue;
      const size_t q = (size_t)f.roots[(size_t)gi];
      const double s = len0[(size_t)gi] / len1[(size_t)gi];
      for (int e = 0; e < 3; e++) out[3 * i + e] = cs[3 * q + e] + (std::isfinite(s) && s > 0 ? s : 1.0) * (ch[3 * i + e] - ch[3 * q + e]);
    }
    if (ncams > 0) BA_HIP_CHECK(hipMemcpyAsync((double *)w.c[cur ^ 1], out.data(), 3 * nc * sizeof(double), hipMemcpyHostToDevice, st));
    BA_CHECK(BA_LAUNCH(k_transavg_linearise, grid_for(npairs, TA_BLK), TA_BLK, 0, st, ea, w.c[cur ^ 1], w.A[cur ^ 1], w.g[cur ^ 1],
                       w.term[cur ^ 1], w.residual, w.edge_weight));
    BA_CHECK(BA_LAUNCH(k_transavg_sum, 1, TA_BLK, 0, st, (int)npairs, w.term[cur ^ 1], (double *)w.cost + 1));
    ch = out;
  }
  double F1 = 0.0;
  if (npairs > 0) {
    BA_HIP_CHECK(hipMemcpyAsync(residual, w.residual, np * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipMemcpyAsync(edge_weight, w.edge_weight, np * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BA_HIP_CHECK(hipMemcpyAsync(&F1, (double *)w.cost + 1, sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  *iterations = its, *cg_iterations = cg_total;
  if (cost) cost[0] = F0, cost[1] = F1;
  const double nan = std::nan("");
  int64_t cnt[BA_TA_STATES] = {0, 0, 0, 0};
  for (size_t i = 0; i < nc; i++) {
    const int gi = f.component[i];
    const int s = gi < 0 ? BA_TA_ISOLATED : (fx[i] ? BA_TA_FIXED : (f.roots[(size_t)gi] == (int)i ? BA_TA_ROOT : BA_TA_OK));
    status[i] = (uint8_t)s, component[i] = gi, cnt[s]++;
    for (int e = 0; e < 3; e++) c[3 * i + e] = gi < 0 ? nan : ch[3 * i + e];
  }
  for (int s = 0; counts && s < BA_TA_STATES; s++) counts[s] = cnt[s];
  return BA_OK;
}
