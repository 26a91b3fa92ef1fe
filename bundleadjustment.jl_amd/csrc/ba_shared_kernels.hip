// Shared camera intrinsics of the LM solve (ba_lm_set_shared_intrinsics, include/ba_hip.h): calibration groups.
//
// A grouping ties (k1, k2, f) of the members of a group together: x = E z, E copying a group's three values to every member.
// The step solves (E'HE + lambda I) dz = -E'g over z and returns dx = E dz.  Everything keeps the layout of x: a vector over
// z is an x-layout vector whose group entries sit at the group's FIRST member (lowest camera index) with exact zeros at the
// other members' intrinsic entries.
//
// This file holds the entries that set and read the grouping of a handle, its upload, and the kernels of the two solve paths:
//   both   k_grp_reduce / k_grp_expand      E' v and E v on an x-layout camera vector (camera order, or the block rows of S)
//   :PCG   k_grp_blk45                      the z-blocks of the block-Jacobi preconditioner
//   direct k_border_product                 SB = S_full E_g from the assembled tiles (all 3G columns in one pass)
//          k_border_reduce                  C = E_g'(S_full - lambda I)E_g + lambda I and rhs_y = E_g' rhs
//          k_border_mask_vec / k_border_mask_S   B, rhs_a and A: the member rows zeroed / replaced by identity rows and columns
//          k_border_T                       T = C - B'Y and t = rhs_y - B'a0
//          k_border_finish                  Cholesky of T, y = T^-1 t, a = a0 - Y y, and the scatter of E_g y -- one launch
// Every sum is a fixed-order loop or a fixed tree: no atomics.
#include <algorithm>
#include <cstring>

#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

constexpr int SB_T = 256;

// the sum of red[0 .. SB_T) by a fixed tree; every thread of the workgroup calls it, the result is in red[0]
__device__ __forceinline__ void tree_sum(double *red, int tid) {
  __syncthreads();
#pragma unroll
  for (int o = SB_T / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
}

// v <- E'v in place: one workgroup per (group, component); the members' entries are summed (fixed stride and tree) into the
// first member's, the others are set to exactly 0.  row[m]: the index of k1 of member m in v
__global__ __launch_bounds__(SB_T) void k_grp_reduce(const int *__restrict__ gptr, const int *__restrict__ row, double *__restrict__ v) {
  __shared__ double red[SB_T];
  const int tid = threadIdx.x, g = blockIdx.x / 3, comp = blockIdx.x % 3;
  const int m0 = gptr[g], m1 = gptr[g + 1];
  double s = 0;
  for (int m = m0 + tid; m < m1; m += SB_T) s += v[row[m] + comp];
  red[tid] = s;
  tree_sum(red, tid);
  for (int m = m0 + 1 + tid; m < m1; m += SB_T) v[row[m] + comp] = 0.0;
  if (tid == 0) v[row[m0] + comp] = red[0];
}

// v <- E v in place (v over z: the first member's entries to every member)
__global__ __launch_bounds__(SB_T) void k_grp_expand(const int *__restrict__ gptr, const int *__restrict__ row, double *__restrict__ v) {
  const int tid = threadIdx.x, g = blockIdx.x / 3, comp = blockIdx.x % 3;
  const int m0 = gptr[g], m1 = gptr[g + 1];
  const double val = v[row[m0] + comp];
  for (int m = m0 + 1 + tid; m < m1; m += SB_T) v[row[m] + comp] = val;
}

// block-Jacobi preconditioner over z (facto = PCG): per group the 3 x 3 intrinsic blocks of the members' diagonal blocks
// (packed lower 9 x 9, 45 per camera) are summed into the first member's; a non-first member keeps its 6 x 6 pose block and
// gets zeros in its intrinsic rows with a unit diagonal.  row[m] = 9 camera + 6 (camera order)
__global__ __launch_bounds__(SB_T) void k_grp_blk45(const int *__restrict__ gptr, const int *__restrict__ row, double *__restrict__ blk45) {
  __shared__ double red[SB_T];
  const int tid = threadIdx.x, g = blockIdx.x;
  const int m0 = gptr[g], m1 = gptr[g + 1];
  for (int e = 0; e < 6; e++) {
    const int idx = e == 0 ? 27 : (e == 1 ? 34 : (e == 2 ? 35 : 42 + (e - 3)));  // (6,6) (7,6) (7,7) (8,6) (8,7) (8,8)
    double s = 0;
    for (int m = m0 + tid; m < m1; m += SB_T) s += blk45[45 * (int64_t)(row[m] / 9) + idx];
    red[tid] = s;
    tree_sum(red, tid);
    const double total = red[0];
    __syncthreads();
    if (tid == 0) blk45[45 * (int64_t)(row[m0] / 9) + idx] = total;
  }
  __syncthreads();
  for (int m = m0 + 1 + tid; m < m1; m += SB_T) {
    double *b = blk45 + 45 * (int64_t)(row[m] / 9);
    for (int q = 21; q < 45; q++) b[q] = (q == 27 || q == 35 || q == 44) ? 1.0 : 0.0;
  }
}

// element (i, j) of the symmetric S from its packed lower tiles (zero for a tile outside a block-sparse pattern)
__device__ __forceinline__ double s_elem(const double *__restrict__ S, const int64_t *__restrict__ co, int64_t i, int64_t j) {
  const int64_t a = i >= j ? i : j, b = i >= j ? j : i;
  const int64_t tt = tix(co, a / NB, b / NB);
  return tt < 0 ? 0.0 : S[(tt * NB + (a % NB)) * NB + (b % NB)];
}

// SB[k][i] = sum over the members c of group k / 3 of S(i, row[c] + k % 3): thread i of a workgroup row, column k = blockIdx.y.
// Rows n .. npad - 1 (padding) are 0.  The members are added in ascending camera order.
__global__ __launch_bounds__(SB_T) void k_border_product(int64_t n, int64_t npad, const double *__restrict__ S,
                                                          const int64_t *__restrict__ co, const int *__restrict__ gptr,
                                                          const int *__restrict__ row, double *__restrict__ SB) {
  const int64_t i = (int64_t)blockIdx.x * SB_T + threadIdx.x;
  if (i >= npad) return;
  const int k = blockIdx.y, g = k / 3, comp = k % 3;
  double s = 0;
  if (i < n)
    for (int m = gptr[g]; m < gptr[g + 1]; m++) s += s_elem(S, co, i, (int64_t)row[m] + comp);
  SB[(int64_t)k * npad + i] = s;
}

// workgroup (k, l): l < mz: C[k][l] = sum over the members c of group k / 3 of SB[l][row[c] + k % 3], minus lambda (count - 1)
// on the diagonal (the damping acts once per group parameter); l == mz: rhs_y[k] = the same sum over rhs.  out: C (mz x mz,
// row-major) followed by rhs_y (mz)
__global__ __launch_bounds__(SB_T) void k_border_reduce(int64_t npad, int mz, double lambda, const int *__restrict__ gptr,
                                                         const int *__restrict__ row, const double *__restrict__ SB,
                                                         const double *__restrict__ rhs, double *__restrict__ out) {
  __shared__ double red[SB_T];
  const int tid = threadIdx.x, k = blockIdx.x, l = blockIdx.y, g = k / 3, comp = k % 3;
  const int m0 = gptr[g], m1 = gptr[g + 1];
  const double *src = l < mz ? SB + (int64_t)l * npad : rhs;
  double s = 0;
  for (int m = m0 + tid; m < m1; m += SB_T) s += src[row[m] + comp];
  red[tid] = s;
  tree_sum(red, tid);
  if (tid == 0) {
    if (l < mz) out[k * mz + l] = red[0] - (k == l ? lambda * (double)(m1 - m0 - 1) : 0.0);
    else out[mz * mz + k] = red[0];
  }
}

// B = SB with the member rows zeroed, rhs_a = rhs with the member entries zeroed (col[i] >= 0: row i is a member's intrinsic)
__global__ __launch_bounds__(SB_T) void k_border_mask_vec(int64_t npad, int mz, const int *__restrict__ col, double *__restrict__ SB,
                                                           double *__restrict__ rhs) {
  const int64_t i = (int64_t)blockIdx.x * SB_T + threadIdx.x;
  if (i >= npad || col[i] < 0) return;
  rhs[i] = 0.0;
  for (int l = 0; l < mz; l++) SB[(int64_t)l * npad + i] = 0.0;
}

// A: the member rows and columns of S replaced by identity rows and columns.  One workgroup per stored tile, over the
// workspace's list of them as k_scale_S_list (tile t of S is (tiles[t].x, tiles[t].y)); only the masked elements are stored
__global__ __launch_bounds__(SB_T) void k_border_mask_S(int64_t npad, const int *__restrict__ col, double *__restrict__ S,
                                                         const int2 *__restrict__ tiles) {
  __shared__ int any_r, any_c;
  __shared__ signed char mr[NB], mc[NB];
  const int64_t t = blockIdx.x, ti = tiles[t].x, tj = tiles[t].y;
  const int tid = threadIdx.x;
  if (tid == 0) any_r = any_c = 0;
  __syncthreads();
  if (tid < NB) {
    const int64_t r = ti * NB + tid, c = tj * NB + tid;
    mr[tid] = (r < npad && col[r] >= 0) ? 1 : 0;
    mc[tid] = (c < npad && col[c] >= 0) ? 1 : 0;
    if (mr[tid]) any_r = 1;
    if (mc[tid]) any_c = 1;
  }
  __syncthreads();
  if (!any_r && !any_c) return;
  double *T = S + t * NB * NB;
  for (int e = tid; e < NB * NB; e += SB_T) {
    const int r = e >> 7, c = e & (NB - 1);
    if (mr[r] || mc[c]) T[e] = (ti == tj && r == c) ? 1.0 : 0.0;
  }
}

// workgroup (k, l): l < mz: T[k][l] = C[k][l] - sum_i B[k][i] Y[l][i]; l == mz: t[k] = rhs_y[k] - sum_i B[k][i] a0[i].
// cin: C then rhs_y (k_border_reduce); out: T (mz x mz, row-major) then t
__global__ __launch_bounds__(SB_T) void k_border_T(int64_t npad, int mz, const double *__restrict__ B, const double *__restrict__ Y,
                                                    const double *__restrict__ a0, const double *__restrict__ cin,
                                                    double *__restrict__ out) {
  __shared__ double red[SB_T];
  const int tid = threadIdx.x, k = blockIdx.x, l = blockIdx.y;
  const double *bk = B + (int64_t)k * npad, *v = l < mz ? Y + (int64_t)l * npad : a0;
  double s = 0;
  for (int64_t i = tid; i < npad; i += SB_T) s += bk[i] * v[i];
  red[tid] = s;
  tree_sum(red, tid);
  if (tid == 0) {
    const int o = l < mz ? k * mz + l : mz * mz + k;
    out[o] = cin[o] - red[0];
  }
}

// Every workgroup factors T = L L' (mz <= 24: a few hundred operations, cheaper than a launch of its own and a round trip for
// y) and solves T y = t, then updates its SB_T rows of the camera step: a member's intrinsic row receives its group's y
// (the scatter of E_g y: the members of a group get the same bits), every other row a0 - Y y.  A non-positive pivot raises the
// pivot flag (workgroup 0).
constexpr int MZ_MAX = 24;
__global__ __launch_bounds__(SB_T) void k_border_finish(int64_t npad, int mz, const double *__restrict__ Tt, const double *__restrict__ Y,
                                                         const int *__restrict__ col, double *__restrict__ a, int *__restrict__ flag) {
  __shared__ double L[MZ_MAX * MZ_MAX], y[MZ_MAX];
  __shared__ int bad;
  const int tid = threadIdx.x;
  for (int e = tid; e < mz * mz; e += SB_T) L[e] = Tt[e];
  if (tid < mz) y[tid] = Tt[mz * mz + tid];
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int j = 0; j < mz; j++) {
    if (tid == 0) {
      const double d = L[j * mz + j];
      if (!(d > 0.0)) bad = 1;
      L[j * mz + j] = sqrt(d);
    }
    __syncthreads();
    if (tid > j && tid < mz) L[tid * mz + j] /= L[j * mz + j];
    __syncthreads();
    for (int e = tid; e < mz * mz; e += SB_T) {
      const int r = e / mz, c = e - r * mz;
      if (c > j && r >= c) L[e] -= L[r * mz + j] * L[c * mz + j];
    }
    __syncthreads();
  }
  for (int j = 0; j < mz; j++) {  // L w = t
    if (tid == 0) y[j] /= L[j * mz + j];
    __syncthreads();
    if (tid > j && tid < mz) y[tid] -= L[tid * mz + j] * y[j];
    __syncthreads();
  }
  for (int j = mz - 1; j >= 0; j--) {  // L' y = w
    if (tid == 0) y[j] /= L[j * mz + j];
    __syncthreads();
    if (tid < j) y[tid] -= L[j * mz + tid] * y[j];
    __syncthreads();
  }
  // (only when the flag is clear: a 2 left by a hoisted diagonal kernel that gave up must reach the host, which redoes the step)
  if (blockIdx.x == 0 && tid == 0 && bad && flag[0] == 0) flag[0] = 1;
  const int64_t i = (int64_t)blockIdx.x * SB_T + tid;
  if (i >= npad) return;
  const int c = col[i];
  if (c >= 0) {
    a[i] = y[c];
    return;
  }
  double s = a[i];
  for (int l = 0; l < mz; l++) s -= Y[(int64_t)l * npad + i] * y[l];
  a[i] = s;
}

}  // namespace

int launch_grp_reduce(ba_problem *p, const int *d_gptr, const int *d_row, double *d_v, hipStream_t st) {
  ProfScope ps(p, PC_SHARED_BORDER, st);
  return BA_LAUNCH(k_grp_reduce, 3 * p->grp_n, SB_T, 0, st, d_gptr, d_row, d_v);
}

int launch_grp_expand(ba_problem *p, const int *d_gptr, const int *d_row, double *d_v, hipStream_t st) {
  ProfScope ps(p, PC_SHARED_BORDER, st);
  return BA_LAUNCH(k_grp_expand, 3 * p->grp_n, SB_T, 0, st, d_gptr, d_row, d_v);
}

int launch_grp_blk45(ba_problem *p, double *d_blk45, hipStream_t st) {
  ProfScope ps(p, PC_SHARED_BORDER, st);
  return BA_LAUNCH(k_grp_blk45, p->grp_n, SB_T, 0, st, p->grp_ptr, p->grp_row, d_blk45);
}

int launch_border_prepare(ba_problem *p, const DenseLDL *l, int64_t n, double lambda, const int *d_row, const int *d_col, double *d_B,
                          double *d_rhs, double *d_small, hipStream_t st) {
  ProfScope ps(p, PC_SHARED_BORDER, st);
  const int mz = 3 * p->grp_n;
  const int64_t npad = l->n;
  BA_CHECK(BA_LAUNCH(k_border_product, dim3(grid_for(npad, SB_T), mz), SB_T, 0, st, n, npad, l->S, l->col_off, p->grp_ptr, d_row, d_B));
  BA_CHECK(BA_LAUNCH(k_border_reduce, dim3(mz, mz + 1), SB_T, 0, st, npad, mz, lambda, p->grp_ptr, d_row, d_B, d_rhs, d_small));
  BA_CHECK(BA_LAUNCH(k_border_mask_vec, grid_for(npad, SB_T), SB_T, 0, st, npad, mz, d_col, d_B, d_rhs));
  return BA_LAUNCH(k_border_mask_S, (unsigned)l->n_own_tiles, SB_T, 0, st, npad, d_col, l->S, l->own_tiles);
}

int launch_border_finish(ba_problem *p, const DenseLDL *l, const int *d_col, const double *d_B, const double *d_Y, double *d_a,
                         double *d_small, hipStream_t st) {
  ProfScope ps(p, PC_SHARED_SMALL, st);
  const int mz = 3 * p->grp_n;
  const int64_t npad = l->n;
  double *Tt = d_small + (MZ_MAX + 1) * MZ_MAX;
  BA_CHECK(BA_LAUNCH(k_border_T, dim3(mz, mz + 1), SB_T, 0, st, npad, mz, d_B, d_Y, d_a, d_small, Tt));
  return BA_LAUNCH(k_border_finish, grid_for(npad, SB_T), SB_T, 0, st, npad, mz, Tt, d_Y, d_col, d_a, l->flag);
}

// the handle's grouping to the device, once per change (camera order: the vectors of the controller and of :PCG)
int shared_upload(ba_problem *p) {
  if (!p->grp_dirty) return BA_OK;
  if (p->grp_on()) {
    std::vector<int> row(p->h_grp_mem.size());
    for (size_t m = 0; m < row.size(); m++) row[m] = 9 * p->h_grp_mem[m] + 6;
    BA_CHECK(upload(p->grp_ptr, p->h_grp_ptr));
    BA_CHECK(upload(p->grp_row, row));
  }
  p->grp_dirty = false;
  return BA_OK;
}

// What a step or solve checks before its first launch: the members of a group hold bit-identical (k1, k2, f) in xc (the
// camera part of x, 9 per camera) and agree in the mask bits of k1, k2, f (ba_lm_set_fixed)
int shared_check(const ba_problem *p, const double *xc, const char *who) {
  for (int g = 0; g < p->grp_n; g++) {
    const int first = p->h_grp_mem[(size_t)p->h_grp_ptr[(size_t)g]];
    for (int m = p->h_grp_ptr[(size_t)g] + 1; m < p->h_grp_ptr[(size_t)g + 1]; m++) {
      const int c = p->h_grp_mem[(size_t)m];
      if (memcmp(xc + 9 * (size_t)c + 6, xc + 9 * (size_t)first + 6, 3 * sizeof(double)) != 0) {
        ba_set_error("%s: shared intrinsics: camera %d holds other (k1, k2, f) than camera %d, the first member of its group %d "
                     "(the members of a group must be bit-identical in x; see tie_intrinsics)", who, c + 1, first + 1, g + 1);
        return BA_ERR_ARG;
      }
      if (p->fix_ncam > 0 && ((p->h_fix_cam[(size_t)c] ^ p->h_fix_cam[(size_t)first]) & 0x1C0u)) {
        ba_set_error("%s: shared intrinsics: the fixed-parameter mask of camera %d differs from that of camera %d, the first member "
                     "of its group %d, in the bits of k1, k2, f", who, c + 1, first + 1, g + 1);
        return BA_ERR_ARG;
      }
    }
  }
  return BA_OK;
}

extern "C" int ba_lm_set_shared_intrinsics(ba_problem *p, const int32_t *group) {
  if (!p) {
    ba_set_error("ba_lm_set_shared_intrinsics: null handle");
    return BA_ERR_ARG;
  }
  constexpr int G_MAX = MZ_MAX / 3;
  int64_t count[G_MAX + 1] = {};
  int top = 0;
  if (group)
    for (int64_t c = 0; c < p->ncams; c++) {
      if (group[c] < 0 || group[c] > G_MAX) {
        ba_set_error("ba_lm_set_shared_intrinsics: group[%lld] = %d, must be 0 (own intrinsics) or a group 1..%d", (long long)c,
                     (int)group[c], G_MAX);
        return BA_ERR_ARG;
      }
      count[group[c]]++;
      top = std::max(top, (int)group[c]);
    }
  for (int g = 1; g <= top; g++)
    if (count[g] == 0) {
      ba_set_error("ba_lm_set_shared_intrinsics: the labels have a gap: no camera in group %d, but one in group %d", g, top);
      return BA_ERR_ARG;
    }
  // groups with one member are dropped (they behave as label 0), the others renumbered in label order
  int renum[G_MAX + 1] = {}, ng = 0;
  for (int g = 1; g <= top; g++)
    if (count[g] >= 2) renum[g] = ++ng;
  const bool was_on = p->grp_on();
  p->grp_n = ng;
  p->h_grp.clear();
  p->h_grp_ptr.clear();
  p->h_grp_mem.clear();
  if (ng > 0) {
    p->h_grp.resize((size_t)p->ncams);
    p->h_grp_ptr.assign((size_t)ng + 1, 0);
    for (int64_t c = 0; c < p->ncams; c++) {
      p->h_grp[(size_t)c] = renum[group[c]];
      if (renum[group[c]]) p->h_grp_ptr[(size_t)renum[group[c]]]++;
    }
    for (int g = 0; g < ng; g++) p->h_grp_ptr[(size_t)g + 1] += p->h_grp_ptr[(size_t)g];
    p->h_grp_mem.resize((size_t)p->h_grp_ptr[(size_t)ng]);
    std::vector<int> cur(p->h_grp_ptr.begin(), p->h_grp_ptr.end() - 1);
    for (int64_t c = 0; c < p->ncams; c++)
      if (p->h_grp[(size_t)c]) p->h_grp_mem[(size_t)cur[(size_t)p->h_grp[(size_t)c] - 1]++] = (int)c;
  }
  if (ng > 0 || was_on) p->grp_version++;
  p->grp_dirty = ng > 0;
  return BA_OK;
}

extern "C" int ba_lm_get_shared_intrinsics(const ba_problem *p, int *n_groups, int64_t *n_members) {
  if (!p) {
    ba_set_error("ba_lm_get_shared_intrinsics: null handle");
    return BA_ERR_ARG;
  }
  if (n_groups) *n_groups = p->grp_n;
  if (n_members) *n_members = (int64_t)p->h_grp_mem.size();
  return BA_OK;
}
