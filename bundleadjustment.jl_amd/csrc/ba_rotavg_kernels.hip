// Rotation averaging over the view graph (ba_rotation_loops, ba_average_rotations; include/ba_hip.h, "rotation averaging";
// DESIGN §5u): the kernels and the two device entries.  gfx950 only.  The host side of the graph -- the checks on the pair
// list, the CSR adjacency, the spanning forest -- is ba_view_graph.cpp, which needs no device.
// k_rotavg_prepare: one lane per rotation vector, Rodrigues -> nine doubles (72 B per pair; the loop counts and the sweeps read
//   the same table).
// k_rotation_loops: ONE WAVE PER PAIR (a, b).  The lanes stride over the shorter of the two adjacency lists and look each
//   neighbour c up in the other by bisection (the lists are sorted by neighbour); a hit is a triangle: two 3 x 3 products, a
//   trace and a skew norm in registers.  The two counts are reduced across the wave as integers; one writer per output.
// k_rotavg_sweep: ONE WAVE PER CAMERA, a simultaneous update (reads R_in, writes R_out).  The lanes stride over the camera's
//   list; the four sums (omega v, omega) go through the fixed-order wave_sum; lane 0 takes the step.  The largest step of a
//   sweep is an unsigned 64-bit atomicMax on the bits of a non-negative double: the maximum does not depend on the order.
// k_rotavg_edges: one lane per pair: residual, weight and cost term.  k_rotavg_sum: one workgroup, the terms in a fixed order.
// k_rotavg_finish: one lane per camera: the gauge (R <- R R_root' R_root,start in a component without a fixed camera) and the
//   rotation vector.
#include <algorithm>
#include <cmath>

#include "ba_internal.h"
#include "ba_lm_internal.h"  // robust_rho, wave_sum
#include "ba_view_graph.h"

namespace {

#include "ba_refine_dev.h"  // wave_all_sum_int, rotation_vector_reg
#include "ba_rotavg_dev.h"  // 3 x 3 matrices in scalars, Exp and Log

constexpr int RA_BLK = 256, RA_WAVES = RA_BLK / 64;
constexpr int RA_BATCH = 8;  // sweeps between two looks at delta

__global__ __launch_bounds__(RA_BLK) void k_rotavg_prepare(int64_t n, const double *__restrict__ r, double *__restrict__ R) {
  const int64_t i = (int64_t)blockIdx.x * RA_BLK + threadIdx.x;
  if (i >= n) return;
  double M[9];
  rotavg_exp(r[3 * i], r[3 * i + 1], r[3 * i + 2], M);
#pragma unroll
  for (int e = 0; e < 9; e++) R[9 * i + e] = M[e];
}

// the view graph as the kernels read it: camera c's entries [ptr[c], ptr[c + 1]) sorted by neighbour, edge = 2 * pair +
// (0: c is the pair's first camera, 1: its second)
struct RotavgGraph {
  const int *ptr, *nbr, *edge;
};

__global__ __launch_bounds__(RA_BLK) void k_rotation_loops(int npairs, const int *__restrict__ pa, const int *__restrict__ pb,
                                                           const uint8_t *__restrict__ used, RotavgGraph g, const double *__restrict__ Rrel,
                                                           double threshold, int *__restrict__ n_loops, int *__restrict__ support) {
  const int lane = (int)threadIdx.x & 63, k = (int)blockIdx.x * RA_WAVES + ((int)threadIdx.x >> 6);
  if (k >= npairs) return;
  int nl = 0, ns = 0;
  if (used[k]) {
    const int a = pa[k], b = pb[k];
    const int a0 = g.ptr[a], a1 = g.ptr[a + 1], b0 = g.ptr[b], b1 = g.ptr[b + 1];
    const bool swap = b1 - b0 < a1 - a0;  // stride over the shorter list
    const int s0 = swap ? b0 : a0, s1 = swap ? b1 : a1, o0 = swap ? a0 : b0, o1 = swap ? a1 : b1;
    double Rab[9];
    mat3_load(Rrel + 9 * (int64_t)k, false, Rab);
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
        double Rca[9], Rbc[9], M[9], L[9];
        mat3_load(Rrel + 9 * (int64_t)(ea >> 1), (ea & 1) == 0, Rca);  // listed (a, c): R_{c->a} is the transpose
        mat3_load(Rrel + 9 * (int64_t)(eb >> 1), (eb & 1) == 1, Rbc);  // listed (c, b): R_{b->c} is the transpose
        mat3_mul(Rbc, Rab, M);
        mat3_mul(Rca, M, L);
        nl += 1;
        ns += mat3_angle(L) <= threshold ? 1 : 0;
      }
    }
    nl = wave_all_sum_int(nl);
    ns = wave_all_sum_int(ns);
  }
  if (lane == 0) n_loops[k] = nl, support[k] = ns;
}

struct RotavgSweepArgs {
  int ncams;
  RotavgGraph g;             // the kept pairs
  const double *Rrel, *w;    // per pair
  const uint8_t *fixed;      // per camera
  int loss;
  double c2, damping;
};

__global__ __launch_bounds__(RA_BLK) void k_rotavg_sweep(RotavgSweepArgs a, const double *__restrict__ Rin, double *__restrict__ Rout,
                                                         unsigned long long *delta) {
  const int lane = (int)threadIdx.x & 63, i = (int)blockIdx.x * RA_WAVES + ((int)threadIdx.x >> 6);
  if (i >= a.ncams) return;
  double Ri[9];
  mat3_load(Rin + 9 * (int64_t)i, false, Ri);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0;
  const int e1 = a.g.ptr[i + 1];
  for (int e = a.g.ptr[i] + lane; e < e1; e += 64) {
    const int j = a.g.nbr[e], ed = a.g.edge[e], m = ed >> 1;
    double Rji[9], Rj[9], P[9], M[9], v[3], rw;
    mat3_load(a.Rrel + 9 * (int64_t)m, (ed & 1) == 0, Rji);  // listed (i, j): R_{j->i} is the transpose
    mat3_load(Rin + 9 * (int64_t)j, false, Rj);
    mat3_mul(Rji, Rj, P);
    mat3_mul_bt(P, Ri, M);
    rotavg_log(M, v);
    (void)robust_rho(a.loss, (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], a.c2, &rw);
    const double om = a.w[m] * rw;
    s0 += om * v[0], s1 += om * v[1], s2 += om * v[2], sw += om;
  }
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), sw = wave_sum(sw);
  if (lane != 0) return;
  double Ro[9];
  if (a.fixed[i] || !(sw > 0.0)) {
#pragma unroll
    for (int e = 0; e < 9; e++) Ro[e] = Ri[e];
  } else {
    const double d0 = a.damping * (s0 / sw), d1 = a.damping * (s1 / sw), d2 = a.damping * (s2 / sw);
    double E[9];
    rotavg_exp(d0, d1, d2, E);
    mat3_mul(E, Ri, Ro);
    const double dn = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    atomicMax(delta, (unsigned long long)__double_as_longlong(dn));
  }
#pragma unroll
  for (int e = 0; e < 9; e++) Rout[9 * (int64_t)i + e] = Ro[e];
}

struct RotavgEdgeArgs {
  int npairs;
  const int *pa, *pb, *comp;            // per pair its cameras (0-based); per camera its component (-1: none)
  const uint8_t *finite, *kept;         // per pair
  const double *Rrel, *w;
  int loss;
  double c2;
};

// residual: the angle of R_k R_a R_b' for a pair with a finite r inside one component, else NaN; weight: rho' on a kept pair,
// else 0; term: w c^2 rho(theta^2 / c^2) / 2 on a kept pair, else 0
__global__ __launch_bounds__(RA_BLK) void k_rotavg_edges(RotavgEdgeArgs a, const double *__restrict__ R, double *__restrict__ residual,
                                                         double *__restrict__ weight, double *__restrict__ term) {
  const int k = (int)blockIdx.x * RA_BLK + (int)threadIdx.x;
  if (k >= a.npairs) return;
  const int ca = a.pa[k], cb = a.pb[k];
  double th = __longlong_as_double(0x7ff8000000000000ll), rw = 0.0, cost = 0.0;
  if (a.finite[k] && a.comp[ca] >= 0 && a.comp[ca] == a.comp[cb]) {
    double Rk[9], Ra[9], Rb[9], P[9], M[9];
    mat3_load(a.Rrel + 9 * (int64_t)k, false, Rk);
    mat3_load(R + 9 * (int64_t)ca, false, Ra);
    mat3_load(R + 9 * (int64_t)cb, false, Rb);
    mat3_mul(Rk, Ra, P);
    mat3_mul_bt(P, Rb, M);
    th = mat3_angle(M);
    if (a.kept[k]) cost = 0.5 * (a.w[k] * robust_rho(a.loss, th * th, a.c2, &rw));
  }
  residual[k] = th, weight[k] = rw, term[k] = cost;
}

// out[0] <- the sum of n terms in a fixed order: strided partial sums per thread, the tree of a wave, the four waves in order
__global__ __launch_bounds__(RA_BLK) void k_rotavg_sum(int n, const double *__restrict__ term, double *__restrict__ out) {
  __shared__ double part[RA_WAVES];
  const int t = (int)threadIdx.x;
  double s = 0.0;
  for (int k = t; k < n; k += RA_BLK) s += term[k];
  s = wave_sum(s);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) out[0] = ((part[0] + part[1]) + part[2]) + part[3];
}

// root[c]: the root camera of c's component where its gauge is to be restored (no fixed camera in it), else -1
__global__ __launch_bounds__(RA_BLK) void k_rotavg_finish(int ncams, const int *__restrict__ comp, const int *__restrict__ root,
                                                          const double *__restrict__ R, const double *__restrict__ Rstart,
                                                          double *__restrict__ Rout, double *__restrict__ r) {
  const int c = (int)blockIdx.x * RA_BLK + (int)threadIdx.x;
  if (c >= ncams) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double Rc[9], Ro[9], v[3] = {nan, nan, nan};
  mat3_load(R + 9 * (int64_t)c, false, Rc);
#pragma unroll
  for (int e = 0; e < 9; e++) Ro[e] = Rc[e];
  if (comp[c] >= 0) {
    const int q = root[c];
    if (q >= 0) {
      double Rq[9], Rs[9], G[9];
      mat3_load(R + 9 * (int64_t)q, true, Rq);
      mat3_load(Rstart + 9 * (int64_t)q, false, Rs);
      mat3_mul(Rq, Rs, G);
      mat3_mul(Rc, G, Ro);
    }
    rotation_vector_reg(Ro, v);
  }
#pragma unroll
  for (int e = 0; e < 9; e++) Rout[9 * (int64_t)c + e] = Ro[e];
  r[3 * (int64_t)c] = v[0], r[3 * (int64_t)c + 1] = v[1], r[3 * (int64_t)c + 2] = v[2];
}

// what both entries check and upload: the pairs (0-based), "r is finite", used = the caller's (or all) and finite, the table of
// the relative rotations
struct RotavgInput {
  std::vector<int> pa, pb;
  std::vector<uint8_t> finite, used;
};

int rotavg_input(const char *who, ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *r_rel,
                 const uint8_t *used, RotavgInput *in) {
  if (!p || (npairs > 0 && !r_rel)) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  if (view_graph_check(who, p->ncams, npairs, pair_a1, pair_b1)) return BA_ERR_ARG;
  const size_t n = (size_t)npairs;
  in->pa.resize(n), in->pb.resize(n), in->finite.resize(n), in->used.resize(n);
  for (size_t k = 0; k < n; k++) {
    in->pa[k] = (int)pair_a1[k] - 1, in->pb[k] = (int)pair_b1[k] - 1;
    in->finite[k] = std::isfinite(r_rel[3 * k]) && std::isfinite(r_rel[3 * k + 1]) && std::isfinite(r_rel[3 * k + 2]);
    in->used[k] = in->finite[k] && (!used || used[k]);
  }
  return BA_OK;
}

// the pairs, their flags and the table of their rotation matrices on the device
int rotavg_upload(ba_problem *p, const RotavgInput &in, const double *r_rel, hipStream_t st) {
  RotavgWork &w = p->rotavg;
  const int64_t n = (int64_t)in.pa.size();
  BA_CHECK(put(w.pa, in.pa, st));
  BA_CHECK(put(w.pb, in.pb, st));
  BA_CHECK(put(w.used, in.used, st));
  BA_CHECK(grow(w.r_rel, 3 * n));
  BA_CHECK(grow(w.Rrel, 9 * n));
  if (n > 0) BA_HIP_CHECK(hipMemcpyAsync((double *)w.r_rel, r_rel, (size_t)(3 * n) * sizeof(double), hipMemcpyHostToDevice, st));
  return BA_LAUNCH(k_rotavg_prepare, grid_for(n, RA_BLK), RA_BLK, 0, st, n, w.r_rel, w.Rrel);
}

// the CSR adjacency of the pairs with mask != 0 on the device
int rotavg_graph(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *mask, RotavgGraph *g,
                 hipStream_t st) {
  RotavgWork &w = p->rotavg;
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
int rotavg_loops(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const RotavgInput &in, double threshold,
                 int32_t *n_loops, int32_t *support, hipStream_t st) {
  RotavgWork &w = p->rotavg;
  RotavgGraph g;
  BA_CHECK(rotavg_graph(p, npairs, pair_a1, pair_b1, in.used.data(), &g, st));
  BA_CHECK(grow(w.n_loops, npairs));
  BA_CHECK(grow(w.support, npairs));
  {
    ProfScope ps(p, PC_ROTAVG, st);
    BA_CHECK(BA_LAUNCH(k_rotation_loops, grid_for(npairs, RA_WAVES), RA_BLK, 0, st, (int)npairs, w.pa, w.pb, w.used, g, w.Rrel, threshold,
                       w.n_loops, w.support));
  }
  BA_HIP_CHECK(hipMemcpyAsync(n_loops, w.n_loops, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipMemcpyAsync(support, w.support, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

void mat3_mul_host(const double *A, const double *B, double *C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

int rotavg_opts_check(const char *who, const ba_rotavg_opts *in, ba_rotavg_opts *o) {
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
    ba_set_error("%s: f_scale (radians) must be finite and > 0 under a loss that is not linear, got %g", who, o->f_scale);
    return BA_ERR_ARG;
  }
  if (o->loss == BA_LOSS_LINEAR) o->f_scale = 1.0;
  if (o->damping == 0.0) o->damping = 0.8;
  if (!(o->damping > 0 && o->damping <= 1.0)) {
    ba_set_error("%s: damping must lie in (0, 1] (0: 0.8), got %g", who, o->damping);
    return BA_ERR_ARG;
  }
  if (o->max_sweeps <= 0) o->max_sweeps = 1000;
  if (o->max_sweeps > 100000) {
    ba_set_error("%s: max_sweeps must be <= 100000, got %d", who, o->max_sweeps);
    return BA_ERR_ARG;
  }
  if (!std::isfinite(o->xtol)) {
    ba_set_error("%s: xtol (radians) must be finite (<= 0: exactly max_sweeps sweeps), got %g", who, o->xtol);
    return BA_ERR_ARG;
  }
  if (o->loops) {
    if (!(std::isfinite(o->loop_threshold) && o->loop_threshold > 0)) {
      ba_set_error("%s: loop_threshold (radians) must be finite and > 0, got %g", who, o->loop_threshold);
      return BA_ERR_ARG;
    }
    if (o->min_support <= 0) o->min_support = 1;
  }
  return BA_OK;
}

}  // namespace

extern "C" int ba_rotation_loops(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *r_rel,
                                 const uint8_t *used, double threshold, int32_t *n_loops, int32_t *support) {
  const char *who = "ba_rotation_loops";
  if (!(std::isfinite(threshold) && threshold > 0)) {
    ba_set_error("%s: threshold (radians) must be finite and > 0, got %g", who, threshold);
    return BA_ERR_ARG;
  }
  RotavgInput in;
  BA_CHECK(rotavg_input(who, p, npairs, pair_a1, pair_b1, r_rel, used, &in));
  if (npairs > 0 && (!n_loops || !support)) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  if (npairs == 0) return BA_OK;
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  BA_CHECK(rotavg_upload(p, in, r_rel, st));
  return rotavg_loops(p, npairs, pair_a1, pair_b1, in, threshold, n_loops, support, st);
}

extern "C" int ba_average_rotations(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *r_rel,
                                    const double *weights, const uint8_t *used, const double *r0, const uint8_t *fixed,
                                    const ba_rotavg_opts *opts, double *r, uint8_t *status, int32_t *component, uint8_t *kept,
                                    int32_t *n_loops, int32_t *support, double *residual, double *edge_weight, int32_t *sweeps,
                                    double *delta, double *cost, int64_t *counts) {
  const char *who = "ba_average_rotations";
  ba_rotavg_opts o;
  BA_CHECK(rotavg_opts_check(who, opts, &o));
  RotavgInput in;
  BA_CHECK(rotavg_input(who, p, npairs, pair_a1, pair_b1, r_rel, used, &in));
  const int64_t ncams = p->ncams;
  const size_t nc = (size_t)ncams, np = (size_t)npairs;
  if ((ncams > 0 && (!r || !status || !component)) || (npairs > 0 && (!kept || !residual || !edge_weight)) || !sweeps) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  for (size_t k = 0; weights && k < np; k++)
    if (!std::isfinite(weights[k]) || weights[k] < 0) {
      ba_set_error("%s: weights[%lld] = %g: a weight is finite and >= 0", who, (long long)k, weights[k]);
      return BA_ERR_ARG;
    }
  bool any_fixed = false;
  for (size_t c = 0; fixed && c < nc; c++) any_fixed = any_fixed || fixed[c];
  if (any_fixed && !r0) {
    ba_set_error("%s: fixed cameras are held at r0, which is null", who);
    return BA_ERR_ARG;
  }
  if (r0) {
    std::vector<uint8_t> touched(nc, 0);
    for (size_t k = 0; k < np; k++)
      if (in.used[k]) touched[(size_t)in.pa[k]] = touched[(size_t)in.pb[k]] = 1;
    for (size_t c = 0; c < nc; c++)
      if (touched[c] && !(std::isfinite(r0[3 * c]) && std::isfinite(r0[3 * c + 1]) && std::isfinite(r0[3 * c + 2]))) {
        ba_set_error("%s: r0 of camera %lld, which has a used pair, is not finite", who, (long long)c + 1);
        return BA_ERR_ARG;
      }
  }
  BA_HIP_CHECK(hipSetDevice(p->device));
  hipStream_t st = p->stream;
  RotavgWork &w = p->rotavg;
  BA_CHECK(rotavg_upload(p, in, r_rel, st));

  // the loop filter: a pair with triangles, too few of which close, is dropped
  std::vector<uint8_t> keep(in.used);
  std::vector<int32_t> nl, sup;
  if (o.loops && npairs > 0) {
    nl.resize(np), sup.resize(np);
    BA_CHECK(rotavg_loops(p, npairs, pair_a1, pair_b1, in, o.loop_threshold, nl.data(), sup.data(), st));
    for (size_t k = 0; k < np; k++)
      if (keep[k] && nl[k] > 0 && sup[k] < o.min_support) keep[k] = 0;
  }
  for (size_t k = 0; k < np; k++) {
    kept[k] = keep[k];
    if (n_loops) n_loops[k] = o.loops ? nl[k] : 0;
    if (support) support[k] = o.loops ? sup[k] : 0;
  }

  // the forest of the kept pairs: components, roots, and the start where r0 gives none
  ViewForest f;
  view_graph_forest(ncams, npairs, pair_a1, pair_b1, keep.data(), o.loops ? sup.data() : nullptr, weights, fixed, &f);
  std::vector<double> Rs(9 * nc, 0.0);
  for (size_t c = 0; c < nc; c++) Rs[9 * c] = Rs[9 * c + 4] = Rs[9 * c + 8] = 1.0;
  BA_CHECK(grow(w.R[0], 9 * ncams));
  BA_CHECK(grow(w.R[1], 9 * ncams));
  BA_CHECK(grow(w.Rstart, 9 * ncams));
  if (r0) {
    std::vector<double> v0(3 * nc, 0.0);  // (a camera outside the graph: the identity, never read)
    for (size_t c = 0; c < nc; c++)
      if (f.component[c] >= 0) v0[3 * c] = r0[3 * c], v0[3 * c + 1] = r0[3 * c + 1], v0[3 * c + 2] = r0[3 * c + 2];
    BA_CHECK(put(w.r, v0, st));
    BA_CHECK(BA_LAUNCH(k_rotavg_prepare, grid_for(ncams, RA_BLK), RA_BLK, 0, st, ncams, w.r, w.Rstart));
    BA_HIP_CHECK(hipStreamSynchronize(st));
  } else {
    std::vector<double> Rrel(9 * np);
    if (npairs > 0) BA_HIP_CHECK(hipMemcpyAsync(Rrel.data(), w.Rrel, 9 * np * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    for (int c : f.order) {  // R_child = R_{parent -> child} R_parent along the forest, parents first
      const int64_t k = f.parent_pair[(size_t)c];
      if (k < 0) continue;
      double T[9];
      const bool forward = in.pb[(size_t)k] == c;  // listed (parent, child)
      const int par = forward ? in.pa[(size_t)k] : in.pb[(size_t)k];
      for (int e = 0; e < 9; e++) T[e] = forward ? Rrel[9 * (size_t)k + e] : Rrel[9 * (size_t)k + 3 * (e % 3) + e / 3];
      mat3_mul_host(T, &Rs[9 * (size_t)par], &Rs[9 * (size_t)c]);
    }
    BA_HIP_CHECK(hipMemcpyAsync((double *)w.Rstart, Rs.data(), 9 * nc * sizeof(double), hipMemcpyHostToDevice, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
  }
  BA_HIP_CHECK(hipMemcpyAsync((double *)w.R[0], (const double *)w.Rstart, 9 * nc * sizeof(double), hipMemcpyDeviceToDevice, st));

  // per camera: held or not, the component, the root whose gauge is restored; per pair: kept, finite, weight
  std::vector<uint8_t> fx(nc, 0);
  std::vector<int> root(nc, -1);
  std::vector<uint8_t> comp_fixed(f.roots.size(), 0);
  for (size_t c = 0; c < nc; c++)
    if (fixed && fixed[c] && f.component[c] >= 0) fx[c] = 1, comp_fixed[(size_t)f.component[c]] = 1;
  for (size_t c = 0; c < nc; c++)
    if (f.component[c] >= 0 && !comp_fixed[(size_t)f.component[c]]) root[c] = f.roots[(size_t)f.component[c]];
  std::vector<double> wt(np, 1.0);
  for (size_t k = 0; weights && k < np; k++) wt[k] = weights[k];
  BA_CHECK(put(w.fixed, fx, st));
  BA_CHECK(put(w.comp, f.component, st));
  BA_CHECK(put(w.root, root, st));
  BA_CHECK(put(w.kept, keep, st));
  BA_CHECK(put(w.finite, in.finite, st));
  BA_CHECK(put(w.weight, wt, st));
  BA_CHECK(grow(w.residual, npairs));
  BA_CHECK(grow(w.edge_weight, npairs));
  BA_CHECK(grow(w.term, npairs));
  BA_CHECK(grow(w.cost, 2));
  BA_CHECK(grow(w.delta, o.max_sweeps));
  BA_CHECK(grow(w.r, 3 * ncams));
  RotavgGraph g;
  BA_CHECK(rotavg_graph(p, npairs, pair_a1, pair_b1, keep.data(), &g, st));  // (synchronises: the host vectors above end here too)

  const double c2 = o.f_scale * o.f_scale;
  RotavgEdgeArgs ea{(int)npairs, w.pa, w.pb, w.comp, w.finite, w.kept, w.Rrel, w.weight, o.loss, c2};
  RotavgSweepArgs sa{(int)ncams, g, w.Rrel, w.weight, w.fixed, o.loss, c2, o.damping};
  std::vector<double> dl((size_t)o.max_sweeps, 0.0);
  int done = 0, cur = 0;
  {
    ProfScope ps(p, PC_ROTAVG, st);
    BA_CHECK(BA_LAUNCH(k_rotavg_edges, grid_for(npairs, RA_BLK), RA_BLK, 0, st, ea, w.R[0], w.residual, w.edge_weight, w.term));
    BA_CHECK(BA_LAUNCH(k_rotavg_sum, 1, RA_BLK, 0, st, (int)npairs, w.term, w.cost));
    BA_HIP_CHECK(hipMemsetAsync((double *)w.delta, 0, (size_t)o.max_sweeps * sizeof(double), st));
    while (done < o.max_sweeps) {
      const int batch = std::min(RA_BATCH, o.max_sweeps - done);
      for (int s = 0; s < batch; s++, cur ^= 1)
        BA_CHECK(BA_LAUNCH(k_rotavg_sweep, grid_for(ncams, RA_WAVES), RA_BLK, 0, st, sa, w.R[cur], w.R[cur ^ 1],
                           (unsigned long long *)(double *)w.delta + done + s));
      BA_HIP_CHECK(hipMemcpyAsync(dl.data() + done, (double *)w.delta + done, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, st));
      BA_HIP_CHECK(hipStreamSynchronize(st));
      bool stop = false;
      for (int s = 0; s < batch; s++) stop = stop || (o.xtol > 0 && dl[(size_t)(done + s)] <= o.xtol);
      done += batch;
      if (stop) break;
    }
    BA_CHECK(BA_LAUNCH(k_rotavg_finish, grid_for(ncams, RA_BLK), RA_BLK, 0, st, (int)ncams, w.comp, w.root, w.R[cur], w.Rstart, w.R[cur ^ 1],
                       w.r));
    BA_CHECK(BA_LAUNCH(k_rotavg_edges, grid_for(npairs, RA_BLK), RA_BLK, 0, st, ea, w.R[cur ^ 1], w.residual, w.edge_weight, w.term));
    BA_CHECK(BA_LAUNCH(k_rotavg_sum, 1, RA_BLK, 0, st, (int)npairs, w.term, (double *)w.cost + 1));
  }
  double cst[2] = {0.0, 0.0};
  if (ncams > 0) BA_HIP_CHECK(hipMemcpyAsync(r, w.r, 3 * nc * sizeof(double), hipMemcpyDeviceToHost, st));
  if (npairs > 0) {
    BA_HIP_CHECK(hipMemcpyAsync(residual, w.residual, np * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipMemcpyAsync(edge_weight, w.edge_weight, np * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BA_HIP_CHECK(hipMemcpyAsync(cst, w.cost, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  *sweeps = done;
  for (int s = 0; delta && s < done; s++) delta[s] = dl[(size_t)s];
  if (cost) cost[0] = cst[0], cost[1] = cst[1];
  int64_t cnt[BA_RA_STATES] = {0, 0, 0, 0};
  for (size_t c = 0; c < nc; c++) {
    const int g = f.component[c];
    const int s = g < 0 ? BA_RA_ISOLATED : (fx[c] ? BA_RA_FIXED : (f.roots[(size_t)g] == (int)c ? BA_RA_ROOT : BA_RA_OK));
    status[c] = (uint8_t)s, component[c] = g, cnt[s]++;
  }
  for (int s = 0; counts && s < BA_RA_STATES; s++) counts[s] = cnt[s];
  return BA_OK;
}
