// Covariance estimation at a solution (ba_covariance, ba_lm.hip): selected inversion of the factored reduced
// camera matrix on the f64 matrix cores, and the kernels that gather the camera and point blocks of the covariance from it.
//
// After dense_ldl_factor S = L D L' with the strictly lower tiles of S holding L_ik, Linv holding L_kk^-1 (unit lower, whole
// tile) and D the pivots.  Z = S^-1 is formed tile column by tile column, k = nt-1 down to 0, by the block Takahashi
// recurrence, in place over L:
//   Q_b    = (L_jk L_kk^-1)'                          j = rows[b], the tile rows of column k  (panel buffer V, slot b)
//   Z_ik   = - sum_b Z_ij Q_b'                         i, j in rows      (Z_ij for j > i is Z_ji', read transposed)
//   Z_kk   = L_kk^-T D_k^-1 L_kk^-1 - sum_b Q_b Z_jk   (the whole diagonal tile, symmetrised)
// Dense S: rows = k+1 .. nt-1.  Block-sparse S: the pair's row list of the symbolic factorisation ({k+1} + U_q for column
// 2q, U_q for 2q+1); every tile Z_ij with i, j in that list is in the pattern (the fill holds U_q x U_q), so Z is formed
// on the pattern only.  The sums that are long (early columns) are split over several workgroups whose partial tiles are
// added in a fixed order: no atomics, the same bits on every call.
#include "ba_lm_internal.h"

#include <algorithm>
#include <cmath>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int CKC = 16;       // K chunk staged through LDS
constexpr int CLD = NB + 16;  // LDS operands stored k-major, row stride 144 doubles = 288 dwords: 32 mod 64 banks, so the two
                              // half-waves of an operand read (16 rows x 2 k each) hit disjoint banks
constexpr int CT = 256;       // threads of the tile kernels: 4 waves, wave w owns the 64 x 64 quadrant (w >> 1, w & 1)
constexpr int COV_WG_TARGET = 512;  // workgroups a split sum aims for (two per CU)

// chunk [k0, k0 + CKC) of op(X) into registers: op(X)[r][k] = X[k][r] when tr, else X[r][k] (X: row-major 128 x 128 tile).
// Both forms read 16-byte pieces along the tile's rows (coalesced); 8 doubles per thread.
__device__ __forceinline__ void cov_load(const double *__restrict__ X, bool tr, int k0, d2 v[4]) {
  const int tid = threadIdx.x;
  if (tr) {
#pragma unroll
    for (int it = 0; it < 4; it++) v[it] = *reinterpret_cast<const d2 *>(X + (int64_t)(k0 + (tid >> 6) + 4 * it) * NB + 2 * (tid & 63));
  } else {
#pragma unroll
    for (int it = 0; it < 4; it++) v[it] = *reinterpret_cast<const d2 *>(X + (int64_t)((tid >> 3) + 32 * it) * NB + k0 + 2 * (tid & 7));
  }
}

// ... and into LDS, k-major (s[k * CLD + r]); dk (optional): op(X)[r][k] / dk[k]
__device__ __forceinline__ void cov_stage(double *s, bool tr, const d2 v[4], const double *__restrict__ dk) {
  const int tid = threadIdx.x;
  if (tr) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int kk = (tid >> 6) + 4 * it;
      d2 x = v[it];
      if (dk) {
        const double q = 1.0 / dk[kk];
        x.x *= q;
        x.y *= q;
      }
      *reinterpret_cast<d2 *>(s + kk * CLD + 2 * (tid & 63)) = x;
    }
  } else {
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int r = (tid >> 3) + 32 * it, kp = 2 * (tid & 7);
      s[kp * CLD + r] = dk ? v[it].x / dk[kp] : v[it].x;
      s[(kp + 1) * CLD + r] = dk ? v[it].y / dk[kp + 1] : v[it].y;
    }
  }
}

// acc += op(A) op(B)' over one 128-deep tile on v_mfma_f64_16x16x4f64; dA (optional): op(A)'s columns divided by dA[k].
// One LDS buffer per operand, two barriers per chunk; the next chunk's loads are in flight while this one is multiplied.
__device__ __forceinline__ void cov_tile_acc(const double *__restrict__ A, bool tA, const double *__restrict__ B, bool tB,
                                             const double *__restrict__ dA, double *sA, double *sB, d4 acc[4][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = (wv >> 1) * 64, wc = (wv & 1) * 64;
  const int fr = lane & 15, fk = lane >> 4;
  d2 pa[4], pb[4];
  cov_load(A, tA, 0, pa);
  cov_load(B, tB, 0, pb);
  for (int ch = 0; ch < NB / CKC; ch++) {
    __syncthreads();  // everybody has finished reading the previous chunk
    cov_stage(sA, tA, pa, dA ? dA + ch * CKC : nullptr);
    cov_stage(sB, tB, pb, nullptr);
    __syncthreads();
    if (ch + 1 < NB / CKC) {
      cov_load(A, tA, (ch + 1) * CKC, pa);
      cov_load(B, tB, (ch + 1) * CKC, pb);
    }
#pragma unroll
    for (int kk = 0; kk < CKC / 4; kk++) {
      double af[4], bf[4];
#pragma unroll
      for (int m = 0; m < 4; m++) af[m] = sA[(4 * kk + fk) * CLD + wr + 16 * m + fr];
#pragma unroll
      for (int n = 0; n < 4; n++) bf[n] = sB[(4 * kk + fk) * CLD + wc + 16 * n + fr];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int n = 0; n < 4; n++) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[n], acc[m][n], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ void cov_zero(d4 acc[4][4]) {
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int n = 0; n < 4; n++) acc[m][n] = (d4){0, 0, 0, 0};
}

// C <- sign * acc (the f64 MFMA's C map: row (lane >> 4) + 4 g, column lane & 15 of each 16 x 16 block)
__device__ __forceinline__ void cov_store(double *__restrict__ C, const d4 acc[4][4], double sign) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = (wv >> 1) * 64, wc = (wv & 1) * 64;
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int n = 0; n < 4; n++)
#pragma unroll
      for (int g = 0; g < 4; g++) C[(wr + 16 * m + (lane >> 4) + 4 * g) * NB + wc + 16 * n + (lane & 15)] = sign * acc[m][n][g];
}

__device__ __forceinline__ double *tile_at(double *S, const int64_t *__restrict__ co, int64_t i, int64_t j) {
  return S + tix(co, i, j) * NB * NB;
}

// B_k^-1 = L_kk^-T D_k^-1 L_kk^-1 of every diagonal tile, into that tile (the factorisation leaves the slot unread)
__global__ __launch_bounds__(CT) void k_cov_binv(double *__restrict__ S, const int64_t *__restrict__ co, const double *__restrict__ Linv,
                                                 const double *__restrict__ D) {
  __shared__ __attribute__((aligned(16))) double sA[CKC * CLD], sB[CKC * CLD];
  const int k = blockIdx.x;
  const double *Lk = Linv + (int64_t)k * NB * NB;
  d4 acc[4][4];
  cov_zero(acc);
  cov_tile_acc(Lk, true, Lk, true, D + (int64_t)k * NB, sA, sB, acc);
  cov_store(tile_at(S, co, k, k), acc, 1.0);
}

// Q_b = L_kk^-T L_jk' (j = rows[b]) into panel slot b
__global__ __launch_bounds__(CT) void k_cov_panel(const double *__restrict__ S, const int64_t *__restrict__ co,
                                                  const double *__restrict__ Linv_k, const int *__restrict__ rows, int k,
                                                  double *__restrict__ V) {
  __shared__ __attribute__((aligned(16))) double sA[CKC * CLD], sB[CKC * CLD];
  const int b = blockIdx.x;
  d4 acc[4][4];
  cov_zero(acc);
  cov_tile_acc(Linv_k, true, S + tix(co, rows[b], k) * NB * NB, false, nullptr, sA, sB, acc);
  cov_store(V + (int64_t)b * NB * NB, acc, 1.0);
}

// the bulk: Z_ik = -sum_b Z_ij Q_b' for i = rows[a], j = rows[b]; workgroup (a, c) sums b in [c ch, (c + 1) ch).  One chunk
// (nch == 1): straight into tile (i, k); else the partial tile goes to part[a nch + c] (k_cov_col_sum adds them up)
__global__ __launch_bounds__(CT, 2) void k_cov_col(double *__restrict__ S, const int64_t *__restrict__ co, const int *__restrict__ rows,
                                                   int m, int k, const double *__restrict__ V, int nch, int ch,
                                                   double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double sA[CKC * CLD], sB[CKC * CLD];
  const int a = blockIdx.x / nch, c = blockIdx.x % nch;
  const int i = rows[a];
  const int b0 = c * ch, b1 = min(m, b0 + ch);
  d4 acc[4][4];
  cov_zero(acc);
  for (int b = b0; b < b1; b++) {
    const int j = rows[b];
    const bool tr = j > i;  // Z_ij = Z_ji' above the diagonal (S holds the lower tiles)
    cov_tile_acc(S + (tr ? tix(co, j, i) : tix(co, i, j)) * NB * NB, tr, V + (int64_t)b * NB * NB, false, nullptr, sA, sB, acc);
  }
  if (nch == 1) cov_store(S + tix(co, i, k) * NB * NB, acc, -1.0);
  else cov_store(part + (int64_t)blockIdx.x * NB * NB, acc, 1.0);
}

// tile (rows[a], k) = -(sum of its nch partial tiles, in chunk order); 16 workgroups per tile
__global__ __launch_bounds__(CT) void k_cov_col_sum(double *__restrict__ S, const int64_t *__restrict__ co, const int *__restrict__ rows,
                                                    int k, int nch, const double *__restrict__ part) {
  const int a = blockIdx.x >> 4;
  const int e0 = (blockIdx.x & 15) * (NB * NB / 16);
  double *T = S + tix(co, rows[a], k) * NB * NB;
  const double *P = part + (int64_t)a * nch * NB * NB;
#pragma unroll
  for (int u = 0; u < NB * NB / 16 / CT; u++) {
    const int e = e0 + threadIdx.x + CT * u;
    double v = 0.0;
    for (int c = 0; c < nch; c++) v += P[(int64_t)c * NB * NB + e];
    T[e] = -v;
  }
}

// the diagonal tile's sum: part[c] = sum_b Q_b Z_jk over b in [c ch, (c + 1) ch)
__global__ __launch_bounds__(CT) void k_cov_diag(const double *__restrict__ S, const int64_t *__restrict__ co, const int *__restrict__ rows,
                                                 int m, int k, const double *__restrict__ V, int ch, double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double sA[CKC * CLD], sB[CKC * CLD];
  const int c = blockIdx.x;
  const int b0 = c * ch, b1 = min(m, b0 + ch);
  d4 acc[4][4];
  cov_zero(acc);
  for (int b = b0; b < b1; b++)
    cov_tile_acc(V + (int64_t)b * NB * NB, false, S + tix(co, rows[b], k) * NB * NB, true, nullptr, sA, sB, acc);
  cov_store(part + (int64_t)c * NB * NB, acc, 1.0);
}

// Z_kk = sym(B_k^-1 - sum_c part[c]) over the whole diagonal tile; thread (r, c), r >= c, owns both (r, c) and (c, r)
__global__ __launch_bounds__(CT) void k_cov_diag_sum(double *__restrict__ S, const int64_t *__restrict__ co, int k, int nch,
                                                     const double *__restrict__ part) {
  const int e = blockIdx.x * CT + threadIdx.x;
  const int r = e / NB, c = e % NB;
  if (r < c) return;
  double *T = S + tix(co, k, k) * NB * NB;
  double x = T[r * NB + c], y = T[c * NB + r];
  for (int q = 0; q < nch; q++) {
    x -= part[(int64_t)q * NB * NB + r * NB + c];
    y -= part[(int64_t)q * NB * NB + c * NB + r];
  }
  const double v = 0.5 * (x + y);
  T[r * NB + c] = v;
  T[c * NB + r] = v;
}

// diag(S) of the assembled system (before the factorisation overwrites it)
__global__ __launch_bounds__(CT) void k_cov_sdiag(int64_t n, const double *__restrict__ S, const int64_t *__restrict__ co,
                                                  double *__restrict__ sd) {
  const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (i >= n) return;
  const int64_t t = i / NB, r = i - t * NB;
  sd[i] = S[(tix(co, t, t) * NB + r) * NB + r];
}

// min_i D_i / S_ii over the n camera rows (NaN counts as -inf); one workgroup
__global__ __launch_bounds__(1024) void k_cov_min_ratio(int64_t n, const double *__restrict__ D, const double *__restrict__ sd,
                                                        double *__restrict__ out) {
  __shared__ double red[16];
  double v = INFINITY;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    double q = D[i] / sd[i];
    if (q != q) q = -INFINITY;
    v = fmin(v, q);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = fmin(v, __shfl_xor(v, s, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = red[0];
    for (int w = 1; w < 16; w++) m = fmin(m, red[w]);
    out[0] = m;
  }
}

// element (r, c) of the symmetric Z, lower storage; diagonal tiles hold both triangles
__device__ __forceinline__ double zget(const double *__restrict__ S, const int64_t *__restrict__ co, int64_t r, int64_t c) {
  const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
  const int64_t ti = hi / NB, tj = lo / NB;
  const int64_t t = tix(co, ti, tj);
  if (t < 0) return 0.0;  // outside the pattern: cannot happen for cameras that share a point
  return S[(t * NB + (hi - ti * NB)) * NB + (lo - tj * NB)];
}

// 9 x 9 diagonal block of every camera, in the caller's camera order: block row pos[c] of Z; fixed components 0
__global__ __launch_bounds__(CT) void k_cov_cams(int64_t ncams, const double *__restrict__ S, const int64_t *__restrict__ co,
                                                 const int *__restrict__ pos, const uint16_t *__restrict__ fix_cam,
                                                 double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (e >= 81 * ncams) return;
  const int64_t c = e / 81;
  const int ab = (int)(e - 81 * c), a = ab / 9, b = ab % 9;
  const unsigned fm = fix_cam ? fix_cam[c] : 0u;
  const int64_t r0 = 9 * (int64_t)(pos ? pos[c] : (int)c);
  out[e] = ((fm >> a) & 1u) || ((fm >> b) & 1u) ? 0.0 : zget(S, co, r0 + a, r0 + b);
}

// one wave per point: Sigma_pp = U^-1 + sum_{o, o'} T_o Z_{c(o) c(o')} T_o'',  T_o = Y_o B_o (3 x 9; Y_o = U^-1 A_o', B_o the
// camera half of J_o).  Pairs o >= o' of the point's observations; lane l holds the Z elements l and 64 + l (< 81) of the
// pair's 9 x 9 block and accumulates their share of the 3 x 3 sum; a fixed butterfly adds the lanes.
__global__ __launch_bounds__(CT) void k_cov_points(int64_t npnts, const int *__restrict__ pt_ptr, const int *__restrict__ pt_obs,
                                                   const int *__restrict__ cam0, const int *__restrict__ pos,
                                                   const double *__restrict__ J, const double *__restrict__ Y,
                                                   const double *__restrict__ Uinv, const double *__restrict__ S,
                                                   const int64_t *__restrict__ co, const uint8_t *__restrict__ fix_pnt,
                                                   double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (p >= npnts) return;
  double *o9 = out + 9 * p;
  if (fix_pnt && fix_pnt[p]) {
    if (lane < 9) o9[lane] = 0.0;
    return;
  }
  const int e1 = lane + 64;
  const bool has1 = e1 < 81;
  const int a0 = lane / 9, b0 = lane % 9, a1 = has1 ? e1 / 9 : 0, b1 = has1 ? e1 % 9 : 0;
  double dg[9], of[9];  // same-observation terms; o > o' terms (their transposes are the o < o' terms)
#pragma unroll
  for (int q = 0; q < 9; q++) dg[q] = of[q] = 0.0;
  const int q0 = pt_ptr[p], q1 = pt_ptr[p + 1];
  for (int u = q0; u < q1; u++) {
    const int64_t ou = pt_obs[u];
    const int cu = cam0[ou];
    const int64_t ru = 9 * (int64_t)(pos ? pos[cu] : cu);
    const double *Ju = J + 24 * ou, *Yu = Y + 6 * ou;
    double tu0[3], tu1[3];  // T_u[r][a0], T_u[r][a1]
#pragma unroll
    for (int r = 0; r < 3; r++) {
      tu0[r] = Yu[2 * r] * Ju[3 + a0] + Yu[2 * r + 1] * Ju[15 + a0];
      tu1[r] = has1 ? Yu[2 * r] * Ju[3 + a1] + Yu[2 * r + 1] * Ju[15 + a1] : 0.0;
    }
    for (int v = q0; v <= u; v++) {
      const int64_t ov = pt_obs[v];
      const int cv = cam0[ov];
      const int64_t rv = 9 * (int64_t)(pos ? pos[cv] : cv);
      const double *Jv = J + 24 * ov, *Yv = Y + 6 * ov;
      const double z0 = zget(S, co, ru + a0, rv + b0), z1 = has1 ? zget(S, co, ru + a1, rv + b1) : 0.0;
      double tv0[3], tv1[3];  // T_v[m][b0], T_v[m][b1]
#pragma unroll
      for (int m = 0; m < 3; m++) {
        tv0[m] = z0 * (Yv[2 * m] * Jv[3 + b0] + Yv[2 * m + 1] * Jv[15 + b0]);
        tv1[m] = has1 ? z1 * (Yv[2 * m] * Jv[3 + b1] + Yv[2 * m + 1] * Jv[15 + b1]) : 0.0;
      }
      if (u == v) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int m = 0; m < 3; m++) dg[3 * r + m] += tu0[r] * tv0[m] + tu1[r] * tv1[m];
      } else {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int m = 0; m < 3; m++) of[3 * r + m] += tu0[r] * tv0[m] + tu1[r] * tv1[m];
      }
    }
  }
  double s[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int m = 0; m < 3; m++) s[3 * r + m] = dg[3 * r + m] + of[3 * r + m] + of[3 * m + r];
#pragma unroll
  for (int q = 0; q < 9; q++)
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) s[q] += __shfl_xor(s[q], w, 64);
  const double *U = Uinv + 6 * p;  // packed 00 01 02 11 12 22
  const double u9[9] = {U[0], U[1], U[2], U[1], U[3], U[4], U[2], U[4], U[5]};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int m = 0; m < 3; m++)
      if (lane == 3 * r + m) o9[3 * r + m] = u9[3 * r + m] + 0.5 * (s[3 * r + m] + s[3 * m + r]);
}

unsigned cov_grid(int64_t n, int per) { return std::max(1u, grid_for(n, per)); }

}  // namespace

int launch_cov_sdiag(ba_problem *p, const DenseLDL *w, int64_t n, double *d_sd, double *d_ratio_out, bool after_factor,
                     hipStream_t st) {
  ProfScope ps(p, PC_COV_INV, st);
  if (!after_factor) return BA_LAUNCH(k_cov_sdiag, cov_grid(n, CT), CT, 0, st, n, w->S, w->col_off, d_sd);
  return BA_LAUNCH(k_cov_min_ratio, 1, 1024, 0, st, n, w->D, d_sd, d_ratio_out);
}

int64_t cov_part_tiles(int64_t nt) { return COV_WG_TARGET + nt; }

int dense_ldl_selinv(ba_problem *p, DenseLDL *w, const int *d_iota, double *d_part, hipStream_t st) {
  ProfScope ps(p, PC_COV_INV, st);
  const int nt = (int)w->nt;
  double *S = w->S;
  const int64_t *co = w->col_off;
  const TilePattern *pat = w->sparse ? w->pat : nullptr;
  BA_CHECK(BA_LAUNCH(k_cov_binv, nt, CT, 0, st, S, co, w->Linv, w->D));
  for (int k = nt - 1; k >= 0; k--) {
    const int *rows;
    int m;
    if (pat) {  // {k+1} + U_q for column 2q, U_q for 2q+1
      const int q = k / 2, l0 = pat->prow_ptr[(size_t)q], c1 = pat->prow_ptr[(size_t)q + 1] - l0;
      rows = (k & 1) ? w->prow + l0 + 1 : w->prow + l0;
      m = (k & 1) ? std::max(c1 - 1, 0) : c1;
    } else {
      rows = d_iota + k + 1;
      m = nt - 1 - k;
    }
    int nch2 = 0;
    if (m > 0) {
      BA_CHECK(BA_LAUNCH(k_cov_panel, m, CT, 0, st, S, co, w->Linv + (int64_t)k * NB * NB, rows, k, w->V));
      // split the sums of length m over nch workgroups per output tile: about COV_WG_TARGET workgroups in all
      int nch = std::min(m, std::max(1, (COV_WG_TARGET + m - 1) / m));
      const int ch = (m + nch - 1) / nch;
      nch = (m + ch - 1) / ch;
      BA_CHECK(BA_LAUNCH(k_cov_col, m * nch, CT, 0, st, S, co, rows, m, k, w->V, nch, ch, d_part));
      if (nch > 1) BA_CHECK(BA_LAUNCH(k_cov_col_sum, 16 * m, CT, 0, st, S, co, rows, k, nch, d_part));
      nch2 = std::min(m, 256);
      const int ch2 = (m + nch2 - 1) / nch2;
      nch2 = (m + ch2 - 1) / ch2;
      BA_CHECK(BA_LAUNCH(k_cov_diag, nch2, CT, 0, st, S, co, rows, m, k, w->V, ch2, d_part));
    }
    BA_CHECK(BA_LAUNCH(k_cov_diag_sum, NB * NB / CT, CT, 0, st, S, co, k, nch2, d_part));
  }
  return BA_OK;
}

int launch_cov_cams(ba_problem *p, const DenseLDL *w, const int *d_pos, const uint16_t *d_fix_cam, double *d_out, hipStream_t st) {
  if (p->ncams == 0) return BA_OK;
  ProfScope ps(p, PC_COV_CAMS, st);
  return BA_LAUNCH(k_cov_cams, cov_grid(81 * p->ncams, CT), CT, 0, st, p->ncams, w->S, w->col_off, d_pos, d_fix_cam, d_out);
}

int launch_cov_points(ba_problem *p, const DenseLDL *w, const int *d_pos, const double *d_J, const double *d_Y, const double *d_Uinv,
                      const uint8_t *d_fix_pnt, double *d_out, hipStream_t st) {
  if (p->npnts == 0) return BA_OK;
  ProfScope ps(p, PC_COV_POINTS, st);
  return BA_LAUNCH(k_cov_points, cov_grid(p->npnts, CT / 64), CT, 0, st, p->npnts, p->pt_ptr, p->pt_obs, p->cam0, d_pos, d_J, d_Y, d_Uinv,
                   w->S, w->col_off, d_fix_pnt, d_out);
}
