// Internal: Schur task lists of the LM workspace and launchers of the normal-equation kernels.
#pragma once
#include "ba_internal.h"

constexpr int RED_BLOCKS = 1024;  // fixed number of partial sums => fixed summation tree
// the passes that stream the stored J (k_obs_scale, k_fix_mask): observations per tile = threads per workgroup, and 16-byte
// vectors of J per observation (2 rows of 12 doubles)
constexpr int OBS_TILE = 256;
constexpr int JV = 12;

// Schur task list (built once per problem on the host): all ordered observation pairs (a, b) of one point with
// camera(a) >= camera(b), sorted by (camera(a), camera(b)); key k owns tasks [key_ptr[k], key_ptr[k+1]).
// Every camera has its diagonal key even when it has no observation.
// Long keys (few cameras, many shared points: Dubrovnik-356 has ~80 tasks per key, LadyBug-49 ~70) are split into chunks of
// `chunk` tasks, one wave per chunk, whose partial 9x9 sums are added up in chunk order by a second kernel: one wave per
// key would leave most of the chip idle there (63 k waves of 40 dependent iterations each).  Keys of at most 2 chunks' worth
// of tasks are summed by one wave as before.
struct SchurTasks {
  int64_t nkeys = 0, ntasks = 0;
  DevBuf<int> key_ptr, key_ca, key_cb;                           // device
  DevBuf<int> task_a, task_b;                                     // device
  int chunk = 0;                                                  // tasks per chunk; keys with more than 2 * chunk tasks are split
  int64_t nsplit = 0, nchunks = 0;
  DevBuf<int> skey, skey_c0;                                      // split keys: key id, first chunk (nsplit + 1 entries)
  DevBuf<int> chunk_t0, chunk_t1;                                 // chunks: task range
  DevBuf<double> partial;                                         // nchunks x 81
  std::vector<unsigned char> tile_occ;                            // host: nt x nt lower tile occupancy of S by the keys (before fill)
  // Fill-reducing camera ordering (ba_order.cpp): key_ca / key_cb are BLOCK ROWS of S; cam_of[k] (device; null = identity)
  // is the camera at block row k, pos its inverse.  Only the reduced camera system lives in that order: S, its right-hand
  // side and solution, the column scaling; x, J, Hcc, gc stay in the caller's camera order.
  DevBuf<int> cam_of, pos;
  std::vector<int> h_key_cb, h_skey;                              // host copies (chunked assembly of a distributed run)
};

// one chunk of tile columns of the reduced camera matrix in a distributed run with per-rank ownership of S: the columns
// [owner's local tile range t0 .. t0 + ntiles), the keys whose 9 x 9 blocks touch them, its offset table (negative: not here).
// A rank that holds all of S assembles it as ONE chunk (LMWork::whole): every tile, the workspace's own offset table, no key
// lists -- the kernels then take every key (k_schur_blocks in its run-ahead loop) and every split key
struct SchurChunk {
  int owner = 0;           // -1: a reduce-scatter chunk -- one segment per owner, `seg` tiles each, laid out by rank
  int64_t t0 = 0, ntiles = 0;
  int64_t seg = 0, my_t0 = 0, my_n = 0;  // reduce-scatter chunk: tiles per segment; where this rank's segment goes in its own S
  const int64_t *cco = nullptr;  // device, nt entries (cco_alloc + 1: tix reads the table's head one entry before)
  DevBuf<int64_t> cco_alloc;
  DevBuf<int> keys, skeys;  // device: key ids / indices into the split-key list (empty: all of them)
  int64_t nkeys = 0, nskeys = 0;
};

// c^2 rho(s / c^2) of one observation's squared reprojection error s, and w = rho'(s / c^2) (robust loss, ba_lm_set_loss; c2 =
// c^2).  scipy's functions (least_squares, loss=...), applied per observation.  Inlined everywhere: log1p / atan / sqrt in double
// are ocml code, no call (tests/test_code_objects.py)
__device__ __forceinline__ double robust_rho(int kind, double s, double c2, double *w) {
  const double z = s / c2;
  switch (kind) {
    case BA_LOSS_HUBER:
      if (z <= 1.0) {
        *w = 1.0;
        return c2 * z;
      } else {
        const double sz = sqrt(z);
        *w = 1.0 / sz;
        return c2 * (2.0 * sz - 1.0);
      }
    case BA_LOSS_SOFT_L1: {
      const double t = sqrt(1.0 + z);
      *w = 1.0 / t;
      return c2 * (2.0 * z / (t + 1.0));  // = 2 (sqrt(1 + z) - 1) without the cancellation
    }
    case BA_LOSS_CAUCHY:
      *w = 1.0 / (1.0 + z);
      return c2 * log1p(z);
    case BA_LOSS_ARCTAN:
      *w = 1.0 / (1.0 + z * z);
      return c2 * atan(z);
    default:
      *w = 1.0;
      return s;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// up to eight sums in one launch pair (launch_sumsq_multi): vector, length, destination array and slot; the second kernel (one
// workgroup) can also publish the controller's scalars to pinned host memory once every sum is in place.  Kind of a job:
// SJ_SQUARES sum v_i^2 (n entries); SJ_ROBUST sum c^2 rho(|r_o|^2 / c^2) over n observations of the interleaved residual v
// under (loss, c2); SJ_SUM sum v_i (n entries: the per-block partials of a kernel of its own, e.g. k_obs_scale).  A job
// with acc set ADDS its sum to what the slot holds -- the value a job before it in the same launch, or a kernel before the
// launch, left there (the prior terms, ba_prior_kernels.hip): the jobs are summed one after the other, in order
constexpr int SUMSQ_JOBS = 8;
enum { SJ_SQUARES = 0, SJ_ROBUST = 1, SJ_SUM = 2 };
struct SumsqJobs {
  int count = 0;
  const double *v[SUMSQ_JOBS] = {};
  int64_t n[SUMSQ_JOBS] = {};
  double *out[SUMSQ_JOBS] = {};
  int slot[SUMSQ_JOBS] = {};
  int kind[SUMSQ_JOBS] = {};
  int acc[SUMSQ_JOBS] = {};
  int nb[SUMSQ_JOBS] = {};  // filled by the launcher
  int loss = 0;             // SJ_ROBUST jobs: BA_LOSS_* and c^2
  double c2 = 1.0;
  // publish (optional; as launch_publish): a[0..na) -> ha, b[0..nb2) -> hb, flag[0] -> hflag
  const double *pa = nullptr, *pb = nullptr;
  double *ha = nullptr, *hb = nullptr;
  const int *pflag = nullptr;
  int *hflag = nullptr;
  int na = 0, nb2 = 0;
  // (a job past the last slot is counted, not stored: launch_sumsq_multi refuses a descriptor with count > SUMSQ_JOBS)
  bool add(const double *vec, int64_t len, double *dst, int s) {
    if (count >= SUMSQ_JOBS) {
      count++;
      return false;
    }
    v[count] = vec;
    n[count] = len;
    out[count] = dst;
    slot[count] = s;
    kind[count] = SJ_SQUARES;
    count++;
    return true;
  }
  void add_robust(const double *r, int64_t nobs, double *dst, int s, int loss_, double c2_) {
    if (!add(r, nobs, dst, s)) return;
    kind[count - 1] = SJ_ROBUST;
    loss = loss_;
    c2 = c2_;
  }
  void add_sum(const double *vals, int64_t len, double *dst, int s, bool accumulate = false) {
    if (!add(vals, len, dst, s)) return;
    kind[count - 1] = SJ_SUM;
    acc[count - 1] = accumulate ? 1 : 0;
  }
  void publish(const double *a, int na_, double *h_a, const double *b, int nb_, double *h_b, const int *flag, int *h_flag) {
    pa = a; na = na_; ha = h_a; pb = b; nb2 = nb_; hb = h_b; pflag = flag; hflag = h_flag;
  }
};

// d_lambda (optional device scalar): the damping used is lambda * d_lambda[0] (hipGraph replays, ba_lm.hip)
int launch_schur_prep(ba_problem *p, double lambda, const double *d_Hpp, const double *d_gp, double *d_Uinv,
                      double *d_u, hipStream_t st, const double *d_lambda = nullptr, const double *d_damp = nullptr,
                      double *d_lambda_copy = nullptr /* d_lambda (may be pinned host memory) is copied here */,
                      double *d_zero = nullptr, int64_t nzero = 0 /* cleared on the way */);
// facto_type = Float16 (ba_normal_kernels.hip, k_f16_cols): |J_j|^2 of every column; column scaling + Float16 rounding
int launch_col_sq(ba_problem *p, const double *d_Hpp, const double *d_hdiag, double *d_jn2, hipStream_t st);
int launch_f16_scale(ba_problem *p, double lambda, double mu, const double *d_jn2, const double *d_J, const double *d_r,
                     double *d_dcol, double *d_damp, double *d_Jq, double *d_rq, hipStream_t st);
// (partials: the split keys' partial sums are formed by this launcher -- by exactly one of the two, see ba_normal_kernels.hip)
int launch_schur_pre(ba_problem *p, const SchurTasks *T, const double *d_J, const double *d_Uinv, double *d_Y, hipStream_t st,
                     bool partials);
int launch_schur_chunk(ba_problem *p, const SchurTasks *T, const SchurChunk *c, const double *d_J, const double *d_Y,
                       const double *d_Hcc, double lambda, double *dest, int64_t n, int64_t npad, hipStream_t st,
                       const double *d_lambda, const double *d_damp, bool partials);
int launch_scale_S_list(ba_problem *p, int64_t n, const double *d_dsc, double *d_S, const int2 *d_tiles, int64_t ntiles, hipStream_t st);
int launch_schur_rhs(ba_problem *p, const double *d_J, const double *d_r, const double *d_u, double *d_rhs,
                     hipStream_t st, const int *d_cam_pnt = nullptr, const int *d_pos = nullptr /* block row of a camera */);
int launch_gather_cams(ba_problem *p, const int *d_pos, const double *d_src, double *d_dst, hipStream_t st);
int launch_backsub(ba_problem *p, const double *d_J, const double *d_Uinv, const double *d_u, const double *d_dc,
                   double *d_dp, hipStream_t st, const double *d_r_model = nullptr, double cr = 1.0, double *d_partial = nullptr,
                   double *d_scal = nullptr, int slot = 0, bool *model_done = nullptr);
int launch_model_sq(ba_problem *p, const double *d_J, const double *d_r, const double *d_delta, double *d_partial,
                    double *d_scal, int slot, hipStream_t st, double cr = 1.0);
// d_a[0..na), d_b[0..nb), d_flag[0] (optional) -> pinned host buffers, one launch
int launch_publish(const double *d_a, int na, double *h_a, const double *d_b, int nb, double *h_b, const int *d_flag, int *h_flag,
                   hipStream_t st);
int launch_sumsq_multi(ba_problem *p, SumsqJobs *jobs, double *d_partial_multi /* SUMSQ_JOBS RED_BLOCKS */, hipStream_t st);
// the per-observation pass over r and J (ba_obs_kernels.hip; robust loss, and information: DESIGN §5i), in place.  With
// information on the handle r <- L' r (residual_plain: d_r holds the plain residual; else it is whitened already and stays) and,
// d_J != null, J <- L' J; with_loss: r <- sqrt(w) r and J <- sqrt(w) J on top, w = rho'(z) under the handle's loss from |r^|^2
// (d_w (optional) <- w).  d_partial (optional): per-block partials of sum c^2 rho(z) at d_partial[0, nb) and of |r~|^2 at
// d_partial[RED_BLOCKS, RED_BLOCKS + nb), nb = obs_blocks(nobs): a fixed grid, so a fixed summation tree; they are written
// whenever asked for.  No launch where neither the loss nor the information acts and no partials are asked for.
// info_upload: the handle's factors to the device when they changed (ba_lm_set_obs_info)
int obs_blocks(int64_t nobs);
int launch_obs_scale(ba_problem *p, double *d_r, double *d_J, double *d_w, double *d_partial, bool residual_plain, bool with_loss,
                     hipStream_t st);
int info_upload(ba_problem *p);
// fixed parameters (ba_fixed_kernels.hip): the handle's mask to the device when it changed (ba_lm_set_fixed); zeros into the
// columns of J of the fixed parameters (no launch without a mask)
int fix_upload(ba_problem *p);
int launch_fix_mask(ba_problem *p, double *d_J, hipStream_t st);
// Gaussian priors (ba_prior_kernels.hip): the handle's lists to the device when they changed (ba_lm_set_priors).
// launch_prior_lin: at x, d_k (and H_k of the centre priors) -> p->pri_d / pri_H, d_k'Lambda_k d_k -> p->pri_cost(), and
// H_k'Lambda_k H_k / H_k'Lambda_k d_k ADDED into the diagonal blocks Hpp / Hcc and into gp / gc under the handle's mask.
// launch_prior_step: d_delta != null: (H_k delta_k + d_k)'Lambda_k (H_k delta_k + d_k) at the stored linearisation ->
// p->pri_model(); d_xt != null: d_k'Lambda_k d_k at xt -> p->pri_cost_trial().  No launch for a kind without priors.
// launch_prior_rhs: behind launch_schur_rhs (which forms the camera right-hand side from J and r alone): H_k'Lambda_k d_k of
// the camera and centre priors at the stored linearisation SUBTRACTED from d_rhs; d_pos: camera -> block row (or null).
int prior_upload(ba_problem *p);
int launch_prior_lin(ba_problem *p, const double *d_x, double *d_Hpp, double *d_gp, double *d_Hcc, double *d_gc, hipStream_t st);
int launch_prior_step(ba_problem *p, const double *d_delta, const double *d_xt, hipStream_t st);
int launch_prior_rhs(ba_problem *p, double *d_rhs, const int *d_pos, hipStream_t st);
// shared intrinsics (ba_shared_kernels.hip): the handle's grouping to the device when it changed
// (ba_lm_set_shared_intrinsics); shared_check: what a step or solve refuses about x and the mask (xc: the camera part of x on the
// host).  launch_grp_reduce / _expand: v <- E'v / E v in place on an x-layout camera vector; d_row: the index of k1 of every
// member in v (p->grp_row in camera order, the workspace's table in the order of S).  launch_grp_blk45: the z-blocks of the
// :PCG preconditioner.  launch_border_prepare: from the assembled S_full and rhs (order of S): B (3G columns of stride npad),
// C and rhs_y -> d_small, then S and rhs masked in place (A, rhs_a).  launch_border_finish: from a0 (in d_a) and Y = A^-1 B the
// camera step a + E_g y, in place; a non-positive pivot of T raises l->flag.  d_small: 2 * 25 * 24 doubles.
constexpr int SHARED_SMALL_DOUBLES = 2 * 25 * 24;
int shared_upload(ba_problem *p);
int shared_check(const ba_problem *p, const double *xc, const char *who);
int launch_grp_reduce(ba_problem *p, const int *d_gptr, const int *d_row, double *d_v, hipStream_t st);
int launch_grp_expand(ba_problem *p, const int *d_gptr, const int *d_row, double *d_v, hipStream_t st);
int launch_grp_blk45(ba_problem *p, double *d_blk45, hipStream_t st);
int launch_border_prepare(ba_problem *p, const DenseLDL *l, int64_t n, double lambda, const int *d_row, const int *d_col, double *d_B,
                          double *d_rhs, double *d_small, hipStream_t st);
int launch_border_finish(ba_problem *p, const DenseLDL *l, const int *d_col, const double *d_B, const double *d_Y, double *d_a,
                         double *d_small, hipStream_t st);
// the optional terms together (ba_lm.hip): fix_upload, prior_upload, shared_upload and info_upload
int terms_upload(ba_problem *p);
int launch_axpy(ba_problem *p, int64_t n, const double *d_x, const double *d_d, double *d_y, hipStream_t st);
int launch_hcc_diag(ba_problem *p, const double *d_Hcc, double *d_hdiag, hipStream_t st);
int launch_cam_scale(ba_problem *p, const double *d_hdiag, double add, double *d_dsc, hipStream_t st,
                     const double *d_lambda = nullptr, const int *d_pos = nullptr);
int launch_scale_scalar(ba_problem *p, int64_t n, double *d_v, double alpha, hipStream_t st);
int launch_scale_vec(ba_problem *p, int64_t n, const double *d_s, double *d_v, int divide, hipStream_t st);

// preconditioned conjugate gradients on the reduced camera system (facto = PCG; ba_normal_kernels.hip)
int launch_wuw(ba_problem *p, const double *d_J, const double *d_h, const double *d_Hcc, const double *d_v, double lam, double *d_q,
               hipStream_t st, const int *d_cam_pnt = nullptr);
int launch_cam_pnt(ba_problem *p, int *d_cam_pnt, hipStream_t st);
int launch_schur_diag(ba_problem *p, const double *d_J, const double *d_Uinv, const double *d_Hcc, double *d_blk45, hipStream_t st);
int launch_pcg_factor(ba_problem *p, double lambda, double *d_blk45, int *d_flag, hipStream_t st);
int launch_axpy_s(ba_problem *p, int64_t n, double a, const double *d_x, double *d_y, hipStream_t st);
int launch_cg_alpha(ba_problem *p, int64_t n, const double *d_p, const double *d_q, double *d_cg, hipStream_t st);
int launch_cg_step(ba_problem *p, const double *d_cg, const double *d_L45, const double *d_p, const double *d_q, double *d_x,
                   double *d_r, double *d_z, double *d_partial, int first, hipStream_t st);
int launch_cg_beta_dir(ba_problem *p, int64_t n, const double *d_partial, double *d_cg, const double *d_z, double *d_p, int first,
                       hipStream_t st);
int launch_wtv(ba_problem *p, const double *d_J, const double *d_Uinv, const double *d_v, double *d_h, hipStream_t st);

// covariance at a solution (ba_cov_kernels.hip).  launch_cov_sdiag: before the factorisation diag(S) -> d_sd (n),
// after it min_i D_i / S_ii -> d_ratio_out[0].  dense_ldl_selinv: S^-1 over the factor, in place (on the pattern of a block-sparse
// S); d_iota: 0 .. nt-1 (the row lists of dense columns), d_part: cov_part_tiles(nt) tiles of partial sums.
int launch_cov_sdiag(ba_problem *p, const DenseLDL *w, int64_t n, double *d_sd, double *d_ratio_out, bool after_factor, hipStream_t st);
int64_t cov_part_tiles(int64_t nt);
int dense_ldl_selinv(ba_problem *p, DenseLDL *w, const int *d_iota, double *d_part, hipStream_t st);
// the cameras' 9 x 9 blocks (81 per camera, caller's order; d_pos: block row of a camera, null = identity) and the points'
// 3 x 3 blocks (9 per point) of S^-1; fixed components / points 0 (either mask may be null)
int launch_cov_cams(ba_problem *p, const DenseLDL *w, const int *d_pos, const uint16_t *d_fix_cam, double *d_out, hipStream_t st);
int launch_cov_points(ba_problem *p, const DenseLDL *w, const int *d_pos, const double *d_J, const double *d_Y, const double *d_Uinv,
                      const uint8_t *d_fix_pnt, double *d_out, hipStream_t st);
