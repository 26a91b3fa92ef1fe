/*
 * ba_hip.h -- C ABI of libba_hip.so, the MI355X (gfx950) implementation of the hot path of
 * CelestineAngla/BundleAdjustment.jl.  Plain C types only; every entry returns an int status
 * (BA_OK == 0) and never throws.  ba_last_error() returns the text of the last failure of the
 * calling thread.
 *
 * Each entry names the reference interface it replaces (paths relative to the reference root).
 * Conventions are the reference's own at this boundary:
 *   - indices are 1-based int64 (Julia Int);
 *   - the unknown vector is x = [X_1(3) ... X_npnts(3) ; C_1(9) ... C_ncams(9)], camera
 *     C = (r1,r2,r3,t1,t2,t3,k1,k2,f)                      (src/ReadFiles.jl:29-40);
 *   - pt2d and residuals are interleaved (x,y) per observation;
 *   - Jacobian COO entries: 24 per observation, row-major 2x12 block, column order
 *     [X(3), r(3), t(3), k1, k2, f]                        (src/BALNLPModels.jl:137-153,201).
 * Host-pointer entries copy in/out and keep no caller pointer after returning (the Julia GC may
 * move or free the arrays).  *_dev entries take device pointers (hipMalloc'ed by the caller, e.g.
 * a torch tensor's data_ptr, or by ba_dev_malloc) and enqueue on the given hipStream_t
 * (void* 0 = the handle's own stream) without synchronising.
 */
#ifndef BA_HIP_H
#define BA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  BA_OK = 0,
  BA_ERR_ARG = 1,       /* bad argument (null pointer, index out of range, size mismatch) */
  BA_ERR_HIP = 2,       /* HIP runtime error (no device, out of memory, launch failure) */
  BA_ERR_IO = 3,        /* BAL file missing / malformed / bzip2 runtime missing */
  BA_ERR_ZERO_PIVOT = 4,/* LDL^T met an exactly zero pivot: SQDException, src/ldl_aux.jl:45-47,199 */
  BA_ERR_NAN_STEP = 5,  /* |delta| is NaN: status :exception, src/lm.jl:297-302 */
  BA_ERR_COMM = 6       /* RCCL or the caller's communication hook failed */
};

/* status of a Levenberg-Marquardt run: src/lm.jl:391-405, src/LevenbergMarquardt.jl:370-380 */
enum {
  BA_ST_UNKNOWN = -1,
  BA_ST_SMALL_STEP = 0,
  BA_ST_FIRST_ORDER = 1,
  BA_ST_SMALL_RESIDUAL = 2,
  BA_ST_ACCEPTABLE = 3,
  BA_ST_NEG_PRED = 4,
  BA_ST_EXCEPTION = 5,
  BA_ST_MAX_ITER = 6
};

typedef struct ba_problem ba_problem; /* opaque: device mirrors of one BALNLPModel (src/BALNLPModels.jl:79-88) */

const char *ba_last_error(void);
int ba_device_count(int *n);
/* name/CU count of device `dev` (for logs) */
int ba_device_info(int dev, char *name, size_t name_cap, int *n_cu, size_t *hbm_bytes);

/* ---- BAL reader: readfile(filename, T)  src/ReadFiles.jl:9-53 ------------------------------
 * `path` is a full path to problem-*.txt or problem-*.txt.bz2 (the reference prepends
 * <repo>/Data/, ReadFiles.jl:10; the host shim does that).  Two calls: header, then body into
 * caller-allocated arrays of the sizes the header gave.  Indices come back 1-based, cameras
 * re-ordered from the file's (r,t,f,k1,k2) to (r,t,k1,k2,f) exactly as ReadFiles.jl:32-43.
 * The _f32 twin parses every decimal straight to float (parse(Float32, .), single rounding). */
int ba_read_bal_header(const char *path, int64_t *ncams, int64_t *npnts, int64_t *nobs);
int ba_read_bal(const char *path, int64_t ncams, int64_t npnts, int64_t nobs, int64_t *cam_idx1,
                int64_t *pnt_idx1, double *pt2d, double *x0);
int ba_read_bal_f32(const char *path, int64_t ncams, int64_t npnts, int64_t nobs, int64_t *cam_idx1,
                    int64_t *pnt_idx1, float *pt2d, float *x0);

/* ---- model: BALNLPModel(...)  src/BALNLPModels.jl:91-106 ------------------------------------
 * Copies the index arrays and pt2d to device `device` (int32 0-based mirrors + the point- and
 * camera-sorted observation lists used by the deterministic reductions).  In a multi-GPU run every
 * rank creates its own shard: local observations, local points renumbered 1..npnts_local, ALL
 * cameras (cam_idx1 stays global). */
int ba_problem_create(int device, int64_t ncams, int64_t npnts, int64_t nobs, const int64_t *cam_idx1,
                      const int64_t *pnt_idx1, const double *pt2d, ba_problem **out);
void ba_problem_destroy(ba_problem *p);
int ba_problem_dims(const ba_problem *p, int64_t *ncams, int64_t *npnts, int64_t *nobs, int64_t *nvar,
                    int64_t *nequ, int64_t *nnzj);

/* cons!(nlp, x, cx) == residual!(FeasibilityResidual(nlp), x, r)  src/BALNLPModels.jl:115-122,39-55 */
int ba_residual(ba_problem *p, const double *x, double *r);
int ba_residual_f32(ba_problem *p, const float *x, float *r); /* BALNLPModel(file, Float32) */
/* jac_structure!(nlp, rows, cols)  src/BALNLPModels.jl:125-158 : 24*nobs 1-based int64 each */
int ba_jac_structure(ba_problem *p, int64_t *rows, int64_t *cols);
/* jac_coord!(nlp, x, vals)  src/BALNLPModels.jl:161-206 + src/JacobianByHand.jl:5-101, NaN -> 0 */
int ba_jac_coord(ba_problem *p, const double *x, double *vals);
int ba_jac_coord_f32(ba_problem *p, const float *x, float *vals);
/* J' r from COO values: mul_sparse(cols, rows, vals, r, nnzj, nvar)  src/lma_aux.jl:194-212 as
 * called at src/lm.jl:57,370.  jtr has nvar entries in the layout of x. */
int ba_jtr(ba_problem *p, const double *vals, const double *r, double *jtr);

/* device-resident twins (no host copies, no synchronisation): what bench.py times.  The kernels move 16 bytes per
 * lane: arrays aligned to 16 bytes (any hipMalloc / torch allocation is) run at the quoted rates. */
int ba_residual_dev(ba_problem *p, const double *d_x, double *d_r, void *stream);
int ba_residual_f32_dev(ba_problem *p, const float *d_x, float *d_r, void *stream);
int ba_jac_structure_dev(ba_problem *p, int64_t *d_rows, int64_t *d_cols, void *stream);
int ba_jac_coord_dev(ba_problem *p, const double *d_x, double *d_vals, void *stream);
int ba_jac_coord_f32_dev(ba_problem *p, const float *d_x, float *d_vals, void *stream);
int ba_jtr_dev(ba_problem *p, const double *d_vals, const double *d_r, double *d_jtr, void *stream);

/* small device-memory helpers so that a C / Julia caller needs no HIP binding of its own */
int ba_dev_malloc(ba_problem *p, size_t bytes, void **d_ptr);
int ba_dev_free(ba_problem *p, void *d_ptr);
/* Host <-> device copies, ordered on a stream and complete on return: enqueued on the handle's own stream (the _on forms:
 * on `stream`, a hipStream_t; NULL = the handle's stream) behind the work already enqueued there; the call returns when
 * that stream has drained.  A communication hook (ba_lm_set_comm_hook) that stages through host memory must use the _on
 * forms with the stream it was given: the library's streams are non-blocking, so a copy on any other stream is neither
 * ordered behind the producer of the data nor visible to the kernels the library launches next on `stream`. */
int ba_memcpy_h2d(ba_problem *p, void *d_dst, const void *h_src, size_t bytes);
int ba_memcpy_d2h(ba_problem *p, void *h_dst, const void *d_src, size_t bytes);
int ba_memcpy_h2d_on(ba_problem *p, void *stream, void *d_dst, const void *h_src, size_t bytes);
int ba_memcpy_d2h_on(ba_problem *p, void *stream, void *h_dst, const void *d_src, size_t bytes);
int ba_synchronize(ba_problem *p);

/* ---- Levenberg_Marquardt(model, facto, perm, normalize[, linesearch]; kwargs...) --------------
 * variant 0: src/LevenbergMarquardt.jl:16-385 (what solve_ba.jl runs); variant 1: src/lm.jl:15-418.
 * The linear step (J'J + lambda I) delta = -J' r -- which the reference obtains from a sparse LDL^T
 * (or QR) of the augmented system, src/lm.jl:154-238 -- is solved on the device through the
 * point-eliminated (Schur) reduced camera system and a dense blocked LDL^T on the f64 matrix cores;
 * `facto` and `perm` therefore only select behaviour that survives that change: both :QR and :LDL
 * give the same step; `perm` orders what is left to order, the cameras of the reduced system (its
 * residual rows and points are eliminated first, as AMD orders them).  Negative tolerances / zero
 * parameters mean "the variant's default" (eps-derived, src/lm.jl:20-26 and
 * src/LevenbergMarquardt.jl:21-26). */
typedef struct ba_lm_opts {
  int variant;    /* 0 LevenbergMarquardt.jl, 1 lm.jl */
  int facto;      /* 0 :LDL, 1 :QR -- both are served by the same device solve of (J'J + lambda I) delta = -J'r; what
                   *    survives of the branch: inside the line search :QR re-evaluates |J delta + r|^2 (src/lm.jl:273)
                   *    while :LDL uses the recursion of src/lm.jl:277 (they differ for delta_d != 2).
                   *    2 :PCG (an extension, no counterpart in the reference: SURVEY 8f) -- the reduced camera system is
                   *    never formed; block-Jacobi preconditioned conjugate gradients apply it through J (two sweeps per
                   *    iteration) to |residual| <= pcg_tol |right-hand side|: an inexact LM step, judged by the same
                   *    accept test; Float64, no column scaling, model value as :QR.  normalize != :None and an explicit
                   *    facto_type = Float32 on a Float64 model are refused (BA_ERR_ARG), not ignored */
  int normalize;  /* 0 :None, 1 :J, 2 :A  (src/lma_aux.jl:102-178) */
  int linesearch; /* lm.jl only, src/lm.jl:264-295 */
  int facto_type; /* lm.jl only, `facto_type` keyword: 0 = Float64 (the default for a Float64 model), 1 = Float32
                   *    (src/lm.jl:170-173, src/diffprecsions.jl:39-41; the default for a Float32 model), 2 = Float16
                   *    (src/lm.jl:165-169, src/lma_aux.jl:30-95: columns of K scaled by their norms and by mu = 6550,
                   *    entries and right-hand side rounded to Float16, step taken unscaled -- the device rounds the same
                   *    inputs and then eliminates / factors in Float32; :LDL only, one GPU) */
  int ite_max;    /* <0: default (200 / 100) */
  int verbose;    /* 1: print the reference's log columns to stderr */
  int x_f32;      /* 1: eltype(x) = Float32 (a BALNLPModel(file, Float32) run): iterates rounded to Float32, residual and
                   *    Jacobian by the Float32 kernels, eps(Float32)-derived default tolerances; x_inout stays double */
  double restol, satol, srtol, oatol, ortol, atol, rtol; /* <0: default */
  double nu_d, nu_m, lambda, delta_d;                    /* <=0: default (3, 3, 30 | 0.1, 2) */
  double max_time;                                        /* <=0: 3600 (inert in the reference, lm.jl:33,115,382) */
  double pcg_tol;                                         /* facto = 2: relative residual of the CG solve, <=0: 1e-8 */
  int pcg_max_iter;                                       /* facto = 2: CG iterations per LM step, <=0: 1000 */
  int perm;       /* fill-reducing ordering (src/lm.jl:84-88, src/LevenbergMarquardt.jl:106-110): 0 :AMD, 1 :Metis,
                   *    2 the caller's camera numbering.  Applied to the cameras of the reduced camera system
                   *    (ba_schur_ordering); x, J and every vector at this boundary keep the caller's numbering */
} ba_lm_opts;

typedef struct ba_lm_stats {
  int status;  /* BA_ST_* */
  int iter;    /* LM iterations (lm.jl:127 / LevenbergMarquardt.jl:240) */
  int n_accepted, n_rejected;
  int n_residual, n_jacobian, n_factor;
  int n_cg;    /* facto = 2: CG iterations over the whole solve */
  double objective;    /* 1/2 |r|^2 at the returned x (robust loss: f, see ba_lm_set_loss) */
  double dual_feas;    /* |J' r| (lm.jl:415; primal_feas in the old variant, LevenbergMarquardt.jl:384; robust loss: |J~'r~|) */
  double lambda_final;
  double elapsed_s;    /* whole call, host wall clock */
  double loop_s;       /* the while-loop only (what iter / time is quoted on) */
} ba_lm_stats;

/* one log row per iteration, the reference's columns (src/lm.jl:120-121,304):
 * iter, f, delta_f, |J'r|, lambda, |delta|, rho = ared/pred (variant 0: 1/2|dr|^2), accepted(1/0) */
typedef void (*ba_log_cb)(void *ctx, int iter, double f, double df, double norm_jtr, double lambda,
                          double norm_delta, double rho, int accepted);

/* x_inout: nvar doubles, x0 in, solution out (the `x=` keyword of src/lm.jl:20).  Minimises under the handle's loss
 * (ba_lm_set_loss; default linear, 1/2 |r|^2). */
int ba_lm_solve(ba_problem *p, const ba_lm_opts *opts, double *x_inout, ba_lm_stats *stats, ba_log_cb cb,
                void *cb_ctx);
/* the same with the iterate resident on the device (d_x_inout: nvar doubles of device memory, e.g. from ba_dev_malloc): no
 * host <-> device copy of x on either side of the loop.  What bench.py times (inputs resident in HBM when the timed region
 * starts); a host that keeps x in its own memory, as the reference does, calls ba_lm_solve. */
int ba_lm_solve_dev(ba_problem *p, const ba_lm_opts *opts, double *d_x_inout, ba_lm_stats *stats, ba_log_cb cb,
                    void *cb_ctx);

/* ---- multi-GPU: observations sharded by point, cameras replicated --------------------------------
 * One process per GPU.  Every rank creates its own shard (ba_problem_create: local observations and points, ALL
 * cameras) and attaches a communicator BEFORE its first solve.  Per LM iteration the ranks then exchange camera-side
 * data only: short Float64 all-reduces (J'r camera part, diag(J'J), right-hand side, scalars), one reduce per rank of
 * the part of the reduced camera matrix that rank owns, and the broadcast of each factored panel pair from its owner
 * (the dense factorisation is distributed over the tile-column pairs, owner of pair q = q mod world; the triangular
 * solves are replicated).  The reference is single-process: none of this has a counterpart there.
 *   ba_lm_set_comm_rccl : RCCL over xGMI, called directly from the library on its own stream.  Rank 0 obtains the
 *                         128-byte id with ba_comm_get_unique_id and hands it to the other ranks by any means the host
 *                         has (torch.distributed, MPI.jl, a file); the call is collective (ncclCommInitRank).
 *   ba_lm_set_comm_hook : the host carries the data.  op: BA_COMM_ALLREDUCE_F64 (count doubles, sum, in place),
 *                         BA_COMM_REDUCE_F64 / BA_COMM_REDUCE_F32 (count doubles / floats, the sum lands on `root` only,
 *                         in place; the Float32 form carries the reduced camera matrix of facto_type = Float32 runs),
 *                         BA_COMM_BCAST_BYTES (count bytes from `root`), BA_COMM_REDUCE_SCATTER_F64 / _F32 (see the enum).
 *                         d_buf is a device pointer; the operation must
 *                         be ordered after prior work on `stream` and complete (or stream-ordered ON `stream`) on return:
 *                         `stream` is not always the handle's main stream (the distributed factorisation hands its
 *                         panels over on a second, transfer stream while the trailing update runs on the main one), and
 *                         both are hipStreamNonBlocking -- a host-staged hook copies with ba_memcpy_d2h_on /
 *                         ba_memcpy_h2d_on(p, stream, ...), never on the null stream. */
enum { BA_COMM_ALLREDUCE_F64 = 0, BA_COMM_REDUCE_F64 = 1, BA_COMM_BCAST_BYTES = 2, BA_COMM_REDUCE_F32 = 3,
       /* d_buf holds `world` segments of `count` doubles / floats; on return segment `rank` (at d_buf + rank * count)
        * holds the sum of that segment over the ranks, the other segments are unspecified; `root` is unused.  What the
        * assembly of the reduced camera matrix uses: every link of every GPU carries 1 / world of a chunk */
       BA_COMM_REDUCE_SCATTER_F64 = 4, BA_COMM_REDUCE_SCATTER_F32 = 5, BA_COMM_OPS = 6 };
#define BA_COMM_ID_BYTES 128
typedef int (*ba_comm_fn)(void *ctx, int op, void *d_buf, int64_t count, int root, void *stream);
int ba_comm_get_unique_id(void *id_out /* BA_COMM_ID_BYTES */);
int ba_lm_set_comm_rccl(ba_problem *p, int rank, int world, const void *id /* BA_COMM_ID_BYTES */);
int ba_lm_set_comm_hook(ba_problem *p, int rank, int world, ba_comm_fn fn, void *ctx);
/* Layout of the reduced camera matrix S (lower triangle of 128 x 128 tiles, nt = ceil(9 ncams / 128) tile rows) over
 * `world` ranks: tile (i, j), j <= i, sits at tile offset col_off[j] + (i - j); the tile columns are taken in pairs
 * (2q, 2q+1) owned by rank q % world, and rank r's columns fill the contiguous tile range [own_range[r], own_range[r+1]).
 * col_off: nt entries, own_range: world + 1 entries (may be NULL).  Host-only, needs no device. */
int ba_dist_layout(int64_t nt, int world, int64_t *col_off, int64_t *own_range);
/* number of transport calls / bytes handed to the transport since the communicator was attached */
int ba_comm_stats(ba_problem *p, int64_t *calls, int64_t *bytes);
/* the same per operation kind: calls[BA_COMM_OPS], bytes[BA_COMM_OPS], indexed by the BA_COMM_* codes (bytes: what one rank
 * hands to the transport) */
int ba_comm_stats_ops(ba_problem *p, int64_t *calls, int64_t *bytes);

/* ---- single linear step, exposed for parity tests and profiling ------------------------------------
 * From (x, lambda): delta (nvar) solving (J'J + lambda I) delta = -J' r, and pred2 = 1/2 |J delta + r|^2
 * (== 1/2 |delta_r|^2 of the reference's augmented solve, src/lm.jl:229).
 * Under a robust loss of the handle (ba_lm_set_loss) J and r are the reweighted J~ and r~: delta solves
 * (J~'J~ + lambda I) delta = -J~'r~, half_sq_model = 1/2 |J~ delta + r~|^2 and jtr = J~'r~ (the gradient of the robust f). */
int ba_lm_step(ba_problem *p, const double *x, double lambda, double *delta, double *half_sq_model,
               double *jtr /* nvar or NULL */);
/* the same step with facto_type = Float32 (src/lm.jl:170-173, src/diffprecsions.jl:39-41): the reduced camera system is
 * rounded to Float32, factored and solved there; everything else stays Float64.  Robust loss: as ba_lm_step (J~, r~) */
int ba_lm_step_f32(ba_problem *p, const double *x, double lambda, double *delta, double *half_sq_model,
                   double *jtr /* nvar or NULL */);
/* the same step by facto = PCG (see ba_lm_opts.facto): tol / max_iter as pcg_tol / pcg_max_iter; cg_iters_out may be NULL.
 * Robust loss: as ba_lm_step (J~, r~) */
int ba_lm_step_pcg(ba_problem *p, const double *x, double lambda, double tol, int max_iter, double *delta,
                   double *half_sq_model, double *jtr, int *cg_iters_out);

/* Block-sparse reduced camera system.  Cameras that share no point leave empty 9 x 9 blocks in S; the reference's sparse
 * LDL^T exploits that (symbolic phase src/ldl_aux.jl:82-119, numeric :122-201).  The device keeps the sparsity at the
 * granularity of its 128 x 128 tiles: on the first direct solve the tile occupancy of the Schur key list goes through a
 * symbolic factorisation per tile column pair, and when the pattern's trailing updates are at most 60 % of the dense
 * factorisation's, assembly-side zeros are skipped by a list-driven schedule and only the pattern's tiles are allocated
 * (one GPU; BA_SPARSE_S=1 / 0 forces it on / off).  tile_fill: pattern tiles (with fill) / all lower tiles; flop_fill: trailing-update tiles of the pattern / of the
 * dense factorisation; sparse_schedule: 1 when the list schedule is in use.  Valid after the first direct solve. */
int ba_lm_schur_pattern(ba_problem *p, double *tile_fill, double *flop_fill, int *sparse_schedule);

/* ---- fill-reducing camera ordering: `perm` = :AMD / :Metis, src/lm.jl:84-88, consumed by ldl_analyse,
 * src/ldl_aux.jl:246-283 ---------------------------------------------------------------------------------
 * The reference orders the augmented matrix K with AMD.jl or Metis.jl (third-party C libraries, absent here).  On the
 * device the residual rows and the points are eliminated first, in closed form; what remains to be ordered is the camera
 * graph (cameras adjacent when they share a point), and an ordering is judged by the 128 x 128 TILE pattern it leaves.
 * method 0 (:AMD): minimum degree with an elimination-tree postorder; 1 (:Metis): nested dissection by level-structure
 * separators; both also offer reverse Cuthill-McKee sequences (hub cameras deferred) and the caller's numbering, and keep
 * the sequence whose symbolic factorisation is cheapest; 2: the caller's numbering.  Only the reduced camera system is
 * permuted (inside the handle); every array at this boundary keeps the caller's camera numbering.
 *   ba_schur_ordering    : host only, no device: the ordering of a problem and the fill it leaves.  perm1 (ncams, may be
 *                          NULL): perm1[k] = the 1-based camera at block row k of S; tile_fill / flop_fill as
 *                          ba_lm_schur_pattern; block_fill: camera pairs sharing a point / all pairs.
 *   ba_lm_set_ordering   : ordering of the handle's next direct solves (default 0; ba_lm_solve sets it from opts.perm).
 *                          Changing it after a direct solve drops the handle's reduced-system workspace.
 *   ba_lm_schur_ordering : the sequence in use after the first direct solve, and the name of the candidate that won
 *                          (static storage). */
int ba_schur_ordering(int64_t ncams, int64_t npnts, int64_t nobs, const int64_t *cam_idx1, const int64_t *pnt_idx1,
                      int method, int64_t *perm1, double *tile_fill, double *flop_fill, double *block_fill);
int ba_lm_set_ordering(ba_problem *p, int method);
int ba_lm_schur_ordering(ba_problem *p, int64_t *perm1, const char **name);

/* ---- robust loss (an extension: the reference minimises 1/2 |r|^2 only) ------------------------------------------
 * Observation i with the 2-vector residual r_i: s_i = |r_i|^2, z_i = s_i / c^2 (c = scale > 0, pixels: scipy's f_scale),
 * f(x) = 1/2 sum_i c^2 rho(z_i) -- the loss acts on each observation's squared reprojection error, as Ceres' LossFunction
 * does.  rho is scipy's function of the same name: linear z; huber z (z <= 1), 2 sqrt(z) - 1; soft_l1 2 (sqrt(1 + z) - 1);
 * cauchy log1p(z); arctan atan(z).  The LM step is linearised in the first-order (IRLS) form: with w_i = rho'(z_i),
 * r~_i = sqrt(w_i) r_i and J~_i = sqrt(w_i) J_i, so J~'r~ = grad f, and the step solves (J~'J~ + lambda I) delta = -J~'r~
 * (normalize :J / :A scale the columns of J~).  The controller takes ared = f(x) - f(x + delta), pred = 1/2 |r~|^2 -
 * 1/2 |J~ delta + r~|^2; its log's f and |J'r|, stats.objective and stats.dual_feas are the robust f and |J~'r~|.
 *   ba_lm_set_loss : the loss of the handle's next ba_lm_solve / ba_lm_solve_dev / ba_lm_step / _f32 / _pcg (default
 *                    BA_LOSS_LINEAR, which runs exactly the unweighted path).  kind outside BA_LOSS_*, a scale that is not
 *                    finite or <= 0: BA_ERR_ARG.  ba_lm_solve refuses a non-linear loss together with linesearch = 1,
 *                    x_f32 = 1 or facto_type = Float16 (BA_ERR_ARG).
 *   ba_lm_get_loss : what the handle holds.
 *   ba_robust_eval : at x, the weights rho'(z_i) (nobs, the caller's observation order; a weight below 1 marks an observation
 *                    the loss discounts) and f, both under the handle's loss; either output may be NULL.  On a shard (see
 *                    multi-GPU) the local observations only: f is this rank's part of the sum. */
enum { BA_LOSS_LINEAR = 0, BA_LOSS_HUBER, BA_LOSS_SOFT_L1, BA_LOSS_CAUCHY, BA_LOSS_ARCTAN };
int ba_lm_set_loss(ba_problem *p, int kind, double scale);
int ba_lm_get_loss(const ba_problem *p, int *kind, double *scale);
int ba_robust_eval(ba_problem *p, const double *x, double *weights /* nobs or NULL */, double *cost /* or NULL */);

/* ---- fixed parameters (an extension: the reference moves every entry of x) ---------------------------------------
 * Granularity: a point is fixed as a whole (its 3 entries); a camera per component, by a 9-bit mask whose bit b is component
 * b of the camera block in storage order r1 r2 r3 t1 t2 t3 k1 k2 f (Jacobian column 3 + b).
 * The LM entries (ba_lm_step / _f32 / _pcg, ba_lm_solve, ba_lm_solve_dev) minimise over the free entries only: the columns
 * of the fixed parameters are zeroed after every evaluation of J, so their gradient entries and their rows and columns of
 * J'J are exactly 0 (the damping lambda stays on the diagonal) and their step is exactly 0.  The free part of the step
 * solves (J_F'J_F + lambda I) delta_F = -J_F'r.  Fixed entries of x come back bit-identical to the input (x_f32 = 1: the
 * Float32 rounding the model applies to x0); a fixed entry holding -0.0 may come back as +0.0.
 * dual_feas / primal_feas, the log's |J'r| and the jtr output of ba_lm_step are the gradient over the free entries (the
 * fixed entries of jtr are exactly 0).  |x| in the small-step test stays the norm of the whole iterate, fixed entries
 * included: they are part of x.  If every parameter is fixed the solve returns at once: status BA_ST_FIRST_ORDER,
 * iter = 0, x unchanged, objective at x, dual_feas = 0.
 * A fully fixed camera keeps its 9 rows in the reduced camera system: they hold the (scaled) damping on the diagonal and
 * zeros elsewhere, so the factorisation keeps its size.
 * Combines with a robust loss, normalize :J / :A (a zero column keeps the scale 1), the line search, facto_type =
 * Float32, :PCG, both variants, every perm, the block-sparse schedule and several ranks.  ba_lm_solve refuses a mask
 * together with facto_type = Float16 (BA_ERR_ARG).  The model entries (ba_residual, ba_jac_coord, ba_jtr,
 * ba_robust_eval) ignore the mask.
 *   ba_lm_set_fixed : the mask of the handle's next LM steps and solves.  cam_mask: ncams entries, bits 0..8 (NULL: no
 *                     camera component fixed); pnt_fixed: npnts entries, 0 / 1 (NULL: no point fixed).  On a shard (see
 *                     multi-GPU): the shard's own points; every rank passes the same cam_mask.  Both NULL (or nothing
 *                     set) clears the mask: the LM entries then run exactly the unmasked path.  A bit above 8 or a
 *                     pnt_fixed value other than 0 / 1: BA_ERR_ARG.  Host only; uploaded when a step or solve runs.
 *   ba_lm_get_fixed : the number of fixed camera components and of fixed points the handle holds (either may be NULL). */
int ba_lm_set_fixed(ba_problem *p, const uint16_t *cam_mask, const uint8_t *pnt_fixed);
int ba_lm_get_fixed(const ba_problem *p, int64_t *n_fixed_cam_params, int64_t *n_fixed_points);

/* ---- Gaussian priors (an extension: the reference has no soft constraint) ------------------------------------------------
 * Three kinds of prior, each a sparse list of 1-based indices with a mean mu and a symmetric positive semi-definite information
 * matrix Lambda, packed lower triangle row-major (3 x 3: xx xy yy xz yz zz, 6 per prior; 9 x 9: 45 per prior, the packing of the
 * camera blocks, component order r1 r2 r3 t1 t2 t3 k1 k2 f):
 *   point  : h(x) = X_p, the point (mu 3, Lambda 6)                    -- ground control points
 *   camera : h(x) = C_c = (r, t, k1, k2, f), the camera block (mu 9, Lambda 45) -- calibration priors, an earlier solve's posterior
 *   centre : h(x) = c(r, t) = -R(r)' t, the camera centre (mu 3, Lambda 6)     -- GPS positions; R the model's Rodrigues
 *            rotation (theta = |r|, axis r / theta, as the residual evaluates it: no theta -> 0 branch), so P1(r, t, c) = R c + t = 0
 * The objective becomes f(x) = f_obs(x) + 1/2 sum_k d_k' Lambda_k d_k, d_k = h_k(x) - mu_k; f_obs is 1/2 |r|^2 or the robust sum
 * (ba_lm_set_loss): priors are NOT passed through the robust loss.  With H_k = dh_k/dx (the identity for point and camera
 * priors; 3 x 6 on (r, t) for a centre prior, derived by hand, dc/dt = -R') a prior adds H_k' Lambda_k d_k to the gradient,
 * H_k' Lambda_k H_k to the diagonal block of its point or camera in the Gauss-Newton matrix, and 1/2 (H_k delta_k + d_k)'
 * Lambda_k (H_k delta_k + d_k) to the model value of a step.  Only diagonal blocks change: the reduced camera system keeps its
 * pattern.  A zero row and column of Lambda leaves that component unconstrained ("GPS height only" is a valid prior).  A camera
 * may carry a camera prior and a centre prior; an index may appear once per kind.
 * stats.objective, stats.dual_feas, the log's f and |J'r|, the jtr output of ba_lm_step and its half_sq_model all include the
 * prior terms.  Fixed parameters (ba_lm_set_fixed): the columns of H_k of fixed components are zeroed, a fixed point's prior
 * adds nothing to its block and gradient (its cost, a constant, stays in f).  With no prior set every entry runs exactly
 * the launch sequence without priors.
 * Combines with both variants, :LDL / :QR / :PCG, facto_type = Float32, normalize :J / :A, every perm, the block-sparse schedule,
 * robust losses and fixed parameters.  ba_lm_solve refuses priors together with linesearch = 1, x_f32 = 1, facto_type =
 * Float16 or a communicator, and ba_lm_step / _f32 / _pcg refuse them on a handle with a communicator (BA_ERR_ARG; the message
 * names the combination).  ba_covariance includes them (see there): soft constraints make the covariance of a gauge-free scene
 * well defined at lambda = 0, and the blocks it returns, inverted, are the information of a camera or point prior of a later solve.
 *   ba_lm_set_priors : the priors of the handle's next LM steps, solves and covariance calls.  All counts 0 clears them.  Host
 *                      only; uploaded when a step or solve runs.  BA_ERR_ARG (the handle keeps what it had): an index out of
 *                      range or repeated within a kind, a value that is not finite, a negative diagonal entry of Lambda, or
 *                      Lambda_ij^2 > Lambda_ii Lambda_jj.
 *   ba_lm_get_priors : the number of priors of each kind the handle holds (any may be NULL).
 *   ba_prior_eval    : at x, cost = 1/2 sum_k d_k' Lambda_k d_k and d_k' Lambda_k d_k of every prior, kind by kind in the order
 *                      given to ba_lm_set_priors; every output may be NULL.  Ignores the mask. */
int ba_lm_set_priors(ba_problem *p,
                     int64_t n_pnt, const int64_t *pnt_idx1, const double *pnt_mu /* 3 n */, const double *pnt_info /* 6 n */,
                     int64_t n_cam, const int64_t *cam_idx1, const double *cam_mu /* 9 n */, const double *cam_info /* 45 n */,
                     int64_t n_ctr, const int64_t *ctr_idx1, const double *ctr_mu /* 3 n */, const double *ctr_info /* 6 n */);
int ba_lm_get_priors(const ba_problem *p, int64_t *n_pnt, int64_t *n_cam, int64_t *n_ctr);
int ba_prior_eval(ba_problem *p, const double *x, double *cost /* or NULL */,
                  double *chi2_pnt, double *chi2_cam, double *chi2_ctr /* d'Lambda d per prior, each may be NULL */);

/* ---- shared camera intrinsics: calibration groups (an extension: every camera of the reference has its own k1, k2, f) ----
 * One physical camera takes many images: a grouping gives every camera a label, 0 = its own intrinsics, g in 1..G (G <= 8) =
 * member of group g, which shares (k1, k2, f) with the group's other members.  A group with one member is dropped when the
 * grouping is set (it behaves as label 0).  With z = x without the intrinsics of every non-first member ("first": the member
 * with the lowest camera index) and x = E z, E copying a group's three values to all members, the LM entries minimise the
 * handle's objective (1/2 |r|^2 or the robust f, plus the priors, at E z) over z: the step solves
 * (E'HE + lambda I) dz = -E'g, H and g the Gauss-Newton matrix and gradient exactly as ba_lm_step forms them (reweighted,
 * columns of fixed entries zeroed, prior terms added); the damping acts once per group parameter; dx = E dz.
 * Every array keeps the layout of x:
 *   x in     : the members of a group must hold bit-identical (k1, k2, f), else BA_ERR_ARG naming the first offending camera;
 *   x out    : the members come back bit-identical (the same step added to the same value);
 *   jtr, dual_feas, the log's |J'r| : the gradient over z -- a group's summed gradient at its first member's (k1, k2, f),
 *              exactly 0 at the other members' (the convention of fixed entries);
 *   |delta|, |x| of the small-step test : norms of the full x-layout vectors; half_sq_model, stats.objective : at dx = E dz;
 *   fixed parameters : the mask bits of k1, k2, f must agree inside a group, else BA_ERR_ARG; a fixed shared component gets a
 *              zero step and keeps its damping on the diagonal;
 *   priors   : act on x = E z and reduce with E' like everything else: a calibration prior on one member is one on the group.
 * :LDL / :QR (Float64) solve the reduced camera system over z as a bordered system: S is assembled as without a grouping, the
 * 3G columns S E_g come from its tiles in one pass, the members' intrinsic rows and columns of S are replaced by the identity,
 * that matrix is factored by the usual LDL' (handle's ordering, dense or block-sparse schedule), one multi-right-hand-side
 * sweep applies it to the border, and a 3G x 3G Cholesky solve on the device closes the system (a non-positive pivot there:
 * BA_ERR_ZERO_PIVOT).  :PCG applies E'(S - lambda I)E + lambda I by expand / product / reduce with z-blocks in its block-Jacobi
 * preconditioner.  Such steps run unrecorded (no hipGraph replay).
 * Refused (BA_ERR_ARG, the message names the combination): a communicator, facto_type Float32 or Float16, x_f32, normalize
 * :J / :A, linesearch = 1, ba_covariance.  With no grouping set (or all labels 0) every entry runs exactly the launch sequence
 * without one.
 *   ba_lm_set_shared_intrinsics : the grouping of the handle's next LM steps and solves; group: ncams labels, NULL clears.
 *                                 A negative label, a label above 8 or a gap in the labels (group g empty, a higher one not):
 *                                 BA_ERR_ARG.  Host only; uploaded when a step or solve runs.
 *   ba_lm_get_shared_intrinsics : the number of groups kept (two members or more) and of their members (either may be NULL). */
int ba_lm_set_shared_intrinsics(ba_problem *p, const int32_t *group /* ncams; 0 = own, 1..G; NULL clears */);
int ba_lm_get_shared_intrinsics(const ba_problem *p, int *n_groups, int64_t *n_members);

/* ---- per-observation information matrices (an extension: every observation of the reference counts with the identity) ----
 * Observation i carries a symmetric positive semi-definite 2 x 2 information matrix Lambda_i (the inverse covariance of its
 * detection, pixels^-2), factored as Lambda_i = L_i L_i' with L_i lower triangular.  Inside the LM entries (ba_lm_step / _f32 /
 * _pcg, ba_lm_solve, ba_lm_solve_dev, ba_covariance) "the residual" becomes r^_i = L_i' r_i and "the Jacobian" J^_i = L_i' J_i
 * (the two rows of the 2 x 12 block are mixed): the objective is 1/2 sum_i r_i' Lambda_i r_i, under a robust loss
 * 1/2 sum_i c^2 rho(r_i' Lambda_i r_i / c^2) -- the loss sees the Mahalanobis distance, its scale is in units of sigma.  Priors
 * are not affected.  The whitening is linear and per observation, so J^ has the sparsity of J and everything downstream runs
 * unchanged on r^ and J^: the mask, the robust reweighting, both block kinds, the Schur assembly (dense or block-sparse, every
 * perm), facto_type = Float32, :PCG, normalize :J / :A, priors, the shared-intrinsics border, the covariance.  stats.objective,
 * stats.dual_feas, the log's f and |J'r|, the jtr output of ba_lm_step and its half_sq_model are quantities of r^ and J^.
 * Lambda_i = 0 drops the observation; a singular Lambda_i constrains one image direction only.
 * ba_robust_eval honours the array too: its weights are rho'(r_i' Lambda_i r_i / c^2), its cost the objective above (also under
 * the linear loss).  The model entries (ba_residual, ba_jac_coord, ba_jtr) ignore it, as they ignore the mask.
 * Refused (BA_ERR_ARG, the message names the combination): linesearch = 1, x_f32 = 1, facto_type = Float16, a communicator.
 * With nothing set every entry runs exactly the launch sequence without the term.
 *   ba_lm_set_obs_info : the array of the handle's next LM steps, solves, covariance and ba_robust_eval calls: xx xy yy of
 *                        every observation, caller's order; NULL clears.  An array of identities is kept as given.  Host only
 *                        (validated and factored: l00 = sqrt(xx), l10 = xy / l00 (0 when xx = 0), l11 = sqrt(max(yy - l10^2,
 *                        0))); uploaded when a step or solve runs.  BA_ERR_ARG (the handle keeps what it had): a value that is
 *                        not finite, a negative diagonal entry, xy^2 > xx yy.
 *   ba_lm_get_obs_info : n_set = nobs when an array is set, else 0; n_zero = the observations with Lambda = 0 (either may be
 *                        NULL). */
int ba_lm_set_obs_info(ba_problem *p, const double *info3 /* nobs * 3: xx xy yy per observation, caller's order; NULL clears */);
int ba_lm_get_obs_info(const ba_problem *p, int64_t *n_set /* 0 or nobs */, int64_t *n_zero /* observations with Lambda == 0 */);

/* ---- covariance at a solution (an extension: the reference has none) ------------------------------------------------
 * At x, under the handle's loss (ba_lm_set_loss) and mask (ba_lm_set_fixed):  Sigma = (J~_F' J~_F + lambda I)^-1, J~ the
 * Jacobian exactly as ba_lm_step sees it (reweighted under a robust loss, the columns of the fixed entries zeroed), F the free
 * entries.  cam_cov (ncams * 81, or NULL): the 9 x 9 diagonal block of every camera, caller's camera order, row-major, block
 * order r1 r2 r3 t1 t2 t3 k1 k2 f; pnt_cov (npnts * 9, or NULL): the 3 x 3 block of every point, row-major.  Rows and
 * columns of fixed entries are exactly 0.  Sigma is not scaled by a residual variance: callers who want one multiply by the
 * usual sigma^2 = 2 f / (nequ - n_free), f the objective at x (1/2 |r|^2, or the robust f) and n_free the free entries.
 * With priors on the handle (ba_lm_set_priors) it assembles as the step does:  Sigma = (J~_F' J~_F + sum_k H_k' Lambda_k H_k +
 * lambda I)^-1.
 * Both blocks come from the point-eliminated reduced camera matrix S, assembled as the LM step does (damping 1 on the fixed
 * entries, lambda on the free ones) and factored by the Float64 LDL' whatever facto a solve would use (:PCG included), with
 * the handle's camera ordering and schedule (BA_SPARSE_S is honoured).
 * Rank check: diag(S) is kept before the factorisation; min_rel_pivot (or NULL) receives min_i D_i / S_ii over the camera rows.
 * A value at or below rank_tol (< 0: the default 1e-10; 0: no check) means S is numerically singular -- typically the
 * 7-DoF similarity gauge left free -- and the call returns BA_ERR_ZERO_PIVOT (min_rel_pivot is still written); so does an
 * exactly zero pivot.  Fix a gauge (e.g. one camera's pose and one translation component of another) or pass lambda > 0.
 * lambda negative or not finite, rank_tol NaN, a handle with a communicator: BA_ERR_ARG.  The next ba_lm_step / ba_lm_solve
 * on the handle gives the same bits as without this call in between. */
int ba_covariance(ba_problem *p, const double *x, double lambda, double rank_tol,
                  double *cam_cov /* ncams * 81, row-major 9x9 per camera, or NULL */,
                  double *pnt_cov /* npnts * 9, row-major 3x3 per point, or NULL */,
                  double *min_rel_pivot /* or NULL */);
/* ---- points with the cameras held (an extension: the reference has no triangulation and no per-point solve) -------------
 * With every camera entry of x held, point i is an independent least-squares problem in its 3 unknowns: the handle's objective
 * restricted to that point,
 *   f_i(X) = sum_{o in obs(i)} 1/2 c^2 rho(r^_o' r^_o / c^2) + 1/2 (X - mu)' Lambda (X - mu)
 * rho and c from ba_lm_set_loss, r^ = L'r from ba_lm_set_obs_info (the plain r when none is set), the last term only for a point
 * that carries a point prior (ba_lm_set_priors).  A point fixed by ba_lm_set_fixed is skipped (BA_PT_FIXED, its bits unchanged;
 * its cost entries and the BEHIND flag are still evaluated).  Camera masks, camera and centre priors and shared intrinsics
 * concern the cameras only and are ignored here.  No communicator is needed: on a shard (see multi-GPU) the call refines the
 * shard's own points and the counts are local.
 * init = 0 starts from the point in x.  init = 1 triangulates first and does not read the point in x: per observation with
 * Lambda != 0 (otherwise unweighted) the measurement is undistorted by 8 fixed-point iterations of q <- u / (1 + k1 |q|^2 +
 * k2 |q|^4), u = pt2d / f; the ray is d = R'(q_x, q_y, -1) / |.| through the centre c = -R't; X solves sum (I - dd') X =
 * sum (I - dd') c by a 3 x 3 Cholesky.  A pivot <= 1e-12 trace, or fewer than two such observations: BA_PT_DEGENERATE.
 * Iteration (Marquardt, per point): at X, w_o = rho'(z_o), H = sum w J^'J^ (+ Lambda), g = sum w J^'r^ (+ Lambda (X - mu)), J^ the
 * whitened 2 x 3 point block; (H + lambda diag H) delta = -g by a 3 x 3 Cholesky (a failed or non-finite factorisation is a
 * rejection); the step is accepted iff f_i(X + delta) <= f_i(X) (a non-finite cost is rejected), then lambda <- max(lambda / 10,
 * 1e-12), else lambda <- 10 lambda.  States: CONVERGED after an accepted step with |delta| <= xtol (|X| + xtol), X the new point;
 * STALLED when lambda > 1e12; MAX_ITER after max_iter trials; NONFINITE when the cost at the start is not finite (the point is
 * unchanged, no flag); DEGENERATE as above and for a free point without an observation (unchanged, cost entries 0, no flag).
 * BA_PT_BEHIND is OR-ed into the state when at the returned X an observation with Lambda != 0 has P1.z >= 0 (the BAL camera
 * looks down -z: a point in front has P1.z < 0).
 * max_iter < 0: 50; max_iter == 0 evaluates only (cost and flag written; with init = 0 x is untouched, with init = 1 it receives
 * the triangulated points; state MAX_ITER); xtol <= 0: 1e-10; lambda0 <= 0: 1e-4.  xtol or lambda0 not finite, init outside
 * 0 / 1: BA_ERR_ARG.
 * cost[2 i] is f_i at the start (init = 1: at the triangulated point), cost[2 i + 1] at the returned point, never larger.
 * counts[s] = points in state s, counts[BA_PT_STATES] = points flagged BEHIND.  iters_max: the most trials any point took.
 * The camera part of x and every skipped or unchanged point come back bit-identical; two calls give the same bits; the next
 * ba_lm_step / ba_lm_solve on the handle gives the same bits as without this call in between.
 * ba_refine_points_dev: x, status and cost in device memory, enqueued on `stream` (NULL: the handle's); with counts and
 * iters_max both NULL it does not synchronise, otherwise it waits for the stream to hand them over. */
enum { BA_PT_CONVERGED = 0, BA_PT_STALLED = 1, BA_PT_MAX_ITER = 2, BA_PT_FIXED = 3,
       BA_PT_DEGENERATE = 4, BA_PT_NONFINITE = 5, BA_PT_STATES = 6,
       BA_PT_BEHIND = 0x80 /* flag OR-ed into the status */ };
int ba_refine_points(ba_problem *p, double *x_inout /* nvar, host */, int init, int max_iter,
                     double xtol, double lambda0,
                     uint8_t *status /* npnts or NULL */, double *cost /* 2 npnts: before, after; or NULL */,
                     int64_t *counts /* BA_PT_STATES + 1 (last: points flagged BEHIND) or NULL */,
                     int *iters_max /* or NULL */);
int ba_refine_points_dev(ba_problem *p, double *d_x_inout /* nvar, device */, int init, int max_iter,
                         double xtol, double lambda0,
                         uint8_t *d_status /* npnts or NULL */, double *d_cost /* 2 npnts or NULL */,
                         int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */, void *stream);

/* ---- cameras with the points held (an extension: the reference has no resection and no per-camera solve) ------------------
 * The other half of ba_refine_points.  With every point entry of x held, camera c is an independent least-squares problem in at
 * most 9 unknowns: the handle's objective restricted to that camera,
 *   f_c(C) = sum_{o in obs(c)} 1/2 c^2 rho(r^_o' r^_o / c^2) + 1/2 (C - mu)' Lambda_cam (C - mu)
 *            + 1/2 (c(C) - mu')' Lambda_ctr (c(C) - mu')
 * rho and c from ba_lm_set_loss, r^ = L'r from ba_lm_set_obs_info (the plain r when none is set; an observation with Lambda = 0 is
 * dropped), the second term only for a camera that carries a camera prior, the third only for one that carries a centre prior,
 * c(C) = -R(r)'t as in ba_lm_set_priors (nonlinear: re-evaluated at every trial).
 * Honoured: ba_lm_set_fixed -- a masked camera component is held: its step is exactly 0 and its bits come back unchanged; a
 * camera with all 9 components held is skipped (BA_PT_FIXED; its cost entries and the BEHIND flag are still evaluated).  A
 * grouping (ba_lm_set_shared_intrinsics): the (k1, k2, f) of every group member are held for this call as if masked and stay
 * bit-identical -- the tied problem is not separable by camera, a pose-only refit is what a grouping leaves.  Ignored: fixed
 * points and point priors (the points are held here anyway).  A handle with a communicator is refused (BA_ERR_ARG): a camera's
 * observations are spread over the shards.
 * Iteration (Marquardt, per camera): at C, w_o = rho'(z_o), H = sum w J^'J^ (+ Lambda_cam + H_ctr' Lambda_ctr H_ctr), g = sum w J^'r^
 * (+ Lambda_cam (C - mu) + H_ctr' Lambda_ctr (c(C) - mu')), J^ the whitened 2 x 9 camera block, H_ctr = dc/d(r, t); the rows and
 * columns of held components are replaced by the identity and g_j = 0 there; (H + lambda diag H) delta = -g by a 9 x 9 Cholesky
 * (a pivot that is not positive or not finite, or a delta that is not finite, is a rejection); the step is accepted iff
 * f_c(C + delta) <= f_c(C) (a non-finite cost is rejected), then lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.
 * States (the BA_PT_* values): CONVERGED after an accepted step with |D delta| <= xtol (|D C| + xtol), D_j = sqrt(H_jj) of the H
 * that produced the step, 0 on held components, C the new camera -- the block mixes units (f ~ 1e3, k2 ~ 1e-12), D delta is the
 * predicted motion in pixels; STALLED when lambda > 1e12; MAX_ITER after max_iter trials; NONFINITE when the cost at the start
 * is not finite (the camera is unchanged, no flag); DEGENERATE for a camera that is not FIXED and has no observation with
 * Lambda != 0, no camera prior and no centre prior (unchanged, cost entries 0, no flag).  BA_PT_BEHIND is OR-ed into the state
 * when at the returned camera an observation with Lambda != 0 has P1.z >= 0.
 * max_iter < 0: 100; max_iter == 0 evaluates only (cost and flag written, x untouched, state MAX_ITER); xtol <= 0: 1e-10;
 * lambda0 <= 0: 1e-4.  xtol or lambda0 not finite: BA_ERR_ARG.
 * cost[2 c] is f_c at the start, cost[2 c + 1] at the returned camera, never larger.  counts[s] = cameras in state s,
 * counts[BA_PT_STATES] = cameras flagged BEHIND.  iters_max: the most trials any camera took.
 * The point part of x and every camera that is not moved come back bit-identical; a camera's result depends on its own data and
 * the order of its observations only; two calls give the same bits; the next ba_lm_step / ba_lm_solve on the handle gives the
 * same bits as without this call in between.
 * ba_refine_cameras_dev: x, status and cost in device memory, enqueued on `stream` (NULL: the handle's); with counts and
 * iters_max both NULL it does not synchronise, otherwise it waits for the stream to hand them over.
 * Out of scope: Float32, refinement inside the LM loop, the tied (shared-intrinsics) problem over a group, several ranks.  (A
 * pose from scratch is ba_resect_cameras, below.) */
int ba_refine_cameras(ba_problem *p, double *x_inout /* nvar, host */, int max_iter, double xtol, double lambda0,
                      uint8_t *status /* ncams or NULL */, double *cost /* 2 ncams: before, after; or NULL */,
                      int64_t *counts /* BA_PT_STATES + 1 (last: cameras flagged BEHIND) or NULL */, int *iters_max /* or NULL */);
int ba_refine_cameras_dev(ba_problem *p, double *d_x_inout /* nvar, device */, int max_iter, double xtol, double lambda0,
                          uint8_t *d_status /* ncams or NULL */, double *d_cost /* 2 ncams or NULL */,
                          int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */, void *stream);

/* ---- linear camera resection as the start of ba_refine_cameras (an extension: the reference has no resection) --------------
 * ba_refine_cameras started from a closed-form pose per camera, computed on the device from the camera's 2D-3D correspondences:
 * what init = 1 (the triangulation) is to ba_refine_points.  Arguments, results, states, counts and refusals are those of
 * ba_refine_cameras; only the start differs.
 * Which cameras: a camera with all 9 components held is BA_PT_FIXED as before.  A camera with ANY pose component (mask bits 0..5
 * of ba_lm_set_fixed) held is not resected: it starts from x exactly as in ba_refine_cameras and its result has those bits.
 * Every other camera is resected, whatever its pose in x is (NaN included: the pose (r, t) of x is never read).  Held intrinsics
 * (mask bits 6..8, the members of a group) do not prevent it.  Camera priors, centre priors, the loss and the whitening by the
 * information (beyond the Lambda = 0 test) act only in the refinement that follows.
 * The resection of camera c, its intrinsics (k1, k2, f) read from x and held:
 *  1. Every observation o of c with Lambda_o != 0 is used, unweighted.  Its measurement is undistorted as in ba_refine_points:
 *     u = pt2d / f, then 8 iterations of q <- u / (1 + k1 |q|^2 + k2 |q|^4).
 *  2. With P = R X + t the BAL projection gives q = -P.xy / P.z: P.x + q_x P.z = 0 and P.y + q_y P.z = 0, two homogeneous linear
 *     equations in the 12 entries of [R | t].  The points are normalised first (Hartley): X~ = s (X - m), m the mean of the used
 *     points and 1 / s their RMS distance from m (the sums are taken about the first used point of the list, so that none
 *     cancels); the unknown becomes gamma [R / s | R m + t].
 *  3. With h = (X~, 1) the 12 x 12 normal matrix is M = [[S0, 0, Sx], [0, S0, Sy], [Sx, Sy, Sq]], S0 = sum h h', Sx = sum q_x h h',
 *     Sy = sum q_y h h', Sq = sum |q|^2 h h'.
 *  4. The eigenvector of the smallest eigenvalue of M (cyclic Jacobi sweeps), lambda_1 <= ... <= lambda_12.
 *  5. BA_PT_DEGENERATE: fewer than 6 used observations; f not finite or zero; used points that all coincide; a moment that is
 *     not finite; lambda_2 <= 1e-10 lambda_12 (coplanar points and other configurations with a second solution: the counterpart
 *     of the triangulation's "pivot <= 1e-12 trace"); a recovered pose that is not finite.
 *  6. The eigenvector is split into A (3 x 3, rows as found) and b (3), with the sign that puts the majority of the used points
 *     in front (A_3 . X~ + b_3 < 0: the BAL camera looks down -z).  R = U diag(1, 1, det(U V')) V' from A = U Sigma V', the
 *     nearest proper rotation; gamma = s mean(Sigma); t = b / gamma - R m.
 *  7. r from R: theta = atan2(|w| / 2, (tr R - 1) / 2) with w the skew part of R, axis w / |w|; for cos theta < 0 the axis comes
 *     from the diagonal of R + I (sign from w); theta < 1e-12 gives r = (1e-12, 0, 0) -- the model has no theta -> 0 branch and
 *     evaluates NaN at r = 0.
 *  8. The Marquardt iteration of ba_refine_cameras runs unchanged from that pose.
 * A resected camera that is DEGENERATE comes back bit-unchanged, cost entries 0, no BEHIND flag (as a point the triangulation
 * cannot place).  cost[2 c] is f_c at the resected pose.  max_iter == 0 writes the resected pose into x (state MAX_ITER, both
 * cost entries f_c at that pose), as init = 1 with max_iter = 0 writes the triangulated points.  A camera whose cost at the
 * resected pose is not finite is NONFINITE and keeps the resected pose.
 * A camera's result depends on its own data and the order of its observations only (no floating-point atomics); two calls give
 * the same bits; the next ba_lm_step / ba_lm_solve on the handle gives the same bits as without this call in between.  A handle
 * with a communicator is refused (BA_ERR_ARG).
 * Out of scope: outlier rejection inside the linear solve (the robust loss acts in the refinement; the consensus stage in front
 * of this entry is ba_ransac_cameras, below), unknown intrinsics beyond the focal length (an unknown f: ba_resect_cameras_focal,
 * further down; a full 3 x 4 DLT with RQ is not provided), Float32, several ranks, resection inside the LM loop. */
int ba_resect_cameras(ba_problem *p, double *x_inout /* nvar, host */, int max_iter, double xtol, double lambda0,
                      uint8_t *status /* ncams or NULL */, double *cost /* 2 ncams: before, after; or NULL */,
                      int64_t *counts /* BA_PT_STATES + 1 (last: cameras flagged BEHIND) or NULL */, int *iters_max /* or NULL */);
int ba_resect_cameras_dev(ba_problem *p, double *d_x_inout /* nvar, device */, int max_iter, double xtol, double lambda0,
                          uint8_t *d_status /* ncams or NULL */, double *d_cost /* 2 ncams or NULL */,
                          int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */, void *stream);

/* ---- outlier-robust camera resection: RANSAC before the linear pose (an extension) ------------------------------------------
 * ba_resect_cameras with a consensus stage in front.  One wrong 2D-3D correspondence ruins the linear pose (every used
 * observation enters the 12 x 12 normal matrix unweighted) and the robust loss only acts in the refinement that follows.  Here
 * many minimal-sample hypotheses are solved and scored on the device, the best one per camera defines an inlier set, and the
 * linear resection and the Marquardt refinement run on that set only.  The inlier mask comes back to the caller.
 * Options (ba_ransac_opts): threshold tau in pixels, finite and > 0; hypotheses H (<= 0: 128; at most 4096); sample m (<= 0: 6;
 * 6..16); refits (< 0: 2; at most 8); min_inliers (<= 0: max(m, 6); at least 6); seed.  Anything else is BA_ERR_ARG, as are
 * NULL options.  A handle with a communicator is refused, as ba_resect_cameras refuses it.
 * Which cameras: the rules of ba_resect_cameras.  A camera with all nine components held is BA_PT_FIXED; a camera with any pose
 * component held is not attempted and starts from x.  For these: inlier = its used observations, n_inliers = their number,
 * best_hyp = -1.  Every other camera is attempted; its pose in x is never read (NaN is fine).  "Used" means Lambda != 0 under
 * ba_lm_set_obs_info; the information plays no other part in the consensus stage.
 * Sampling (64-bit integer arithmetic only, identical on host and device): mix is splitmix64,
 *   z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 * (mix of 0 is 0xE220A8397B1DCDAF; mix of (that ^ 1) is 0x08B4FDA8C892B50E).  Hypothesis h of a camera of degree d has
 * key = mix of (mix of seed ^ h); draw j = 0, 1, ... gives the position pos = ((mix of (key ^ j) >> 32) * d) >> 32 in the
 * camera's observation list (caller's order).  A draw is skipped if its observation is not used or the position was already
 * taken; the first m accepted positions, in the order of their draws, are the sample; fewer than m after 64 draws makes the
 * hypothesis void.  The camera index does not enter: a camera's result depends on its own data, the order of its list and the
 * options only.  ba_ransac_sample is this sampling alone, on the host (no device): `used` holds `degree` bytes or is NULL (all
 * used), pos receives the n_taken <= m accepted positions (n_taken < m: void); sample <= 0: 6.
 * Hypothesis: the pose of steps 1-7 of ba_resect_cameras applied to the m sampled observations in the order of their draws
 * (the sums are taken about the first of them), intrinsics from x; a degenerate sample makes the hypothesis void.
 * Inlier test: under a pose, observation o is an inlier iff it is used, P1.z < 0, and |project - pt2d|^2 <= tau^2 in raw pixels
 * with the model's own projection.  A comparison with NaN fails.
 * Selection: the score of a hypothesis is its inlier count over the camera's whole list; the best is the largest count, ties to
 * the lowest h.  Without a valid hypothesis, or with a best count < min_inliers, the camera fails: its inlier bytes are 0,
 * n_inliers = the best count (0 if none), best_hyp = that h or -1, state BA_PT_DEGENERATE, bit-unchanged, cost entries 0, no flag.
 * Refits, up to `refits` times: the linear resection on the current set M; the whole list re-scored under that pose gives M';
 * M' is adopted iff |M'| >= |M| and M' != M; otherwise (smaller, equal, or the refit was degenerate) M stays and the camera
 * stops.  The poses of these rounds live in a scratch copy of the cameras, not in x.
 * Finish: ba_resect_cameras with the observations outside the final set treated exactly as Lambda = 0 -- the linear resection on
 * the set, then the Marquardt refinement of ba_refine_cameras on the set under the handle's loss, information, priors, mask and
 * grouping; an outlier raises no BEHIND flag; max_iter == 0 returns the linear pose; states, costs, counts and iters_max as in
 * that entry.  x, status and cost equal, bit for bit, those of ba_resect_cameras on the same handle whose information is the
 * caller's with the outliers' entries set to 0 (the identity on the inliers when the caller set none).
 * Outputs beyond those of ba_resect_cameras, each may be NULL: inlier (nobs bytes 0 / 1, caller's observation order), n_inliers
 * (ncams: the size of the final set) and best_hyp (ncams).  In the _dev form they are device pointers and the call is enqueued
 * on `stream`; it synchronises only to hand over counts / iters_max, as its sibling does.
 * Two calls give the same bits (no floating-point atomics); the next ba_lm_step / ba_lm_solve on the handle gives the same bits
 * as without the call.
 * Out of scope: an adaptive hypothesis count, MSAC / LO-RANSAC scoring, unknown intrinsics beyond the focal
 * length (an unknown f: ba_ransac_cameras_focal, further down), Float32, several ranks.  (Minimal samples of three: ba_ransac_cameras_p3p,
 * further down.) */
typedef struct ba_ransac_opts {
  double threshold;
  int hypotheses, sample, refits, min_inliers;
  uint64_t seed;
} ba_ransac_opts;
int ba_ransac_cameras(ba_problem *p, double *x_inout /* nvar, host */, const ba_ransac_opts *opts, int max_iter, double xtol,
                      double lambda0, uint8_t *status /* ncams or NULL */, double *cost /* 2 ncams or NULL */,
                      int64_t *counts /* BA_PT_STATES + 1 or NULL */, int *iters_max /* or NULL */,
                      uint8_t *inlier /* nobs or NULL */, int32_t *n_inliers /* ncams or NULL */, int32_t *best_hyp /* ncams or NULL */);
int ba_ransac_cameras_dev(ba_problem *p, double *d_x_inout /* nvar, device */, const ba_ransac_opts *opts /* host */, int max_iter,
                          double xtol, double lambda0, uint8_t *d_status /* ncams or NULL */, double *d_cost /* 2 ncams or NULL */,
                          int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */,
                          uint8_t *d_inlier /* nobs or NULL */, int32_t *d_n_inliers /* ncams or NULL */,
                          int32_t *d_best_hyp /* ncams or NULL */, void *stream);
int ba_ransac_sample(uint64_t seed, int hypothesis, int64_t degree, const uint8_t *used /* degree, or NULL: all */, int sample,
                     int64_t *pos /* sample */, int *n_taken);

/* ---- camera resection with unknown focal length: linear stage and RANSAC (an extension) --------------------------------------
 * ba_resect_cameras and ba_ransac_cameras for an image without calibration: f is estimated along with the pose.  The BAL
 * principal point is the origin, so no general RQ decomposition is needed: the same 12 x 12 eigenproblem on raw pixels and one
 * ratio of row norms afterwards.  Signatures, arguments, results, states, counts, defaults and refusals are those of the
 * siblings (ba_ransac_opts unchanged); only what is said here differs.
 * Which cameras run in focal mode: a camera whose pose is free (no mask bit 0..5 held) and whose f is free (mask bit 8 of
 * ba_lm_set_fixed not held and the camera in no group of ba_lm_set_shared_intrinsics).  Every other camera is handled as the
 * sibling handles it, in the same launch: a camera with all 9 components held is BA_PT_FIXED; a camera with a pose component
 * held is not resected and starts from x; a camera with f held or in a group gets the calibrated resection of
 * ba_resect_cameras, intrinsics read from x.  For a focal-mode camera the entries (r, t, f) of x are never read, nor are its
 * free k1, k2: NaN is fine.
 * The resection of a focal-mode camera c:
 *  1. Every observation o of c with Lambda_o != 0 is used, unweighted, with its raw measurement m = pt2d.  The image scale is
 *     a = sqrt(sum |m|^2 / n) over the n used observations; u = m / a.  The measurements are NOT centred: the principal point is
 *     the origin and the structure diag(f, f, 1) must survive.  a not finite or 0: BA_PT_DEGENERATE.
 *  2. The Hartley normalisation of the points, exactly as step 2 of ba_resect_cameras (sums about the first used point).
 *  3. The 12 x 12 normal matrix of step 3 of ba_resect_cameras with q := u, its smallest eigenpair by the same Jacobi sweeps, and
 *     the same degeneracy rules (fewer than 6 used observations; coinciding points; a moment that is not finite;
 *     lambda_2 <= 1e-10 lambda_12).  No undistortion iterations run.
 *  4. The eigenvector is gamma [phi A_1; phi A_2; A_3 | phi b_1, phi b_2, b_3] with [A | b] = [R / s | R m + t] and phi = f / a.
 *     phi = sqrt((|A_1|^2 + |A_2|^2) / (2 |A_3|^2)) from the three rows as found; phi not finite or <= 0: BA_PT_DEGENERATE.
 *     Rows 1 and 2 of A and b_1, b_2 are divided by phi; f^ = a phi.
 *  5. Sign, nearest rotation, gamma, t and the rotation vector as steps 6-7 of ba_resect_cameras.
 *  6. Written: the pose and f = f^; a free k1 or k2 is written as 0; a held k1 or k2 (mask bits 6, 7) keeps its bits -- the
 *     linear stage ignores it (a limitation: with a large held distortion f^ and the pose are only a start for the
 *     refinement).  A DEGENERATE camera comes back bit-unchanged, cost entries 0, no flag.
 *  7. The Marquardt iteration of ba_refine_cameras runs unchanged from that camera: cost[2 c] is f_c at the camera just written;
 *     max_iter == 0 returns the linear pose and f^ (state MAX_ITER); a camera whose cost there is not finite is NONFINITE and
 *     keeps the written values.
 * ba_ransac_cameras_focal: the consensus stage of ba_ransac_cameras with these changes.  Sampling: unchanged.  Hypothesis of a
 * focal-mode camera: steps 1-5 on its m sampled observations in the order of their draws; it keeps its pose and its f^.  Inlier
 * test: the model's own projection under (pose, k1', k2', f^), k' the held value from x or 0 if free.  Selection, ties,
 * min_inliers and the refit rule: unchanged; the refits are focal resections on the current set into the scratch cameras,
 * which then hold f^ and k', and the re-scoring reads the scratch camera's intrinsics.  Finish: ba_resect_cameras_focal with
 * the observations outside the final set treated exactly as Lambda = 0.  x, status and cost equal, bit for bit, those of
 * ba_resect_cameras_focal on the same handle whose information is the caller's with the outliers' entries set to 0.
 * No floating-point atomics; two calls give the same bits; a camera's result depends on its own data and the order of its
 * observations only; the next ba_lm_step / ba_lm_solve on the handle gives the same bits as without the call.  A handle with a
 * communicator is refused (BA_ERR_ARG).  On noisy data the linear f^ is only a start (its relative error is 1e-2 at degree 255
 * and can reach 0.7 at degree 6): the refinement behind it is what makes the estimate, as for the calibrated resection.
 * Out of scope: k1 / k2 estimation in the linear stage, a principal point that is not the origin or a general K by RQ, a second
 * calibrated pass after f^, a minimal P4Pf solver (P3P with the f of x: ba_ransac_cameras_p3p, further down), MSAC or an adaptive hypothesis count, Float32, several ranks, the
 * tied problem over a group. */
int ba_resect_cameras_focal(ba_problem *p, double *x_inout /* nvar, host */, int max_iter, double xtol, double lambda0,
                            uint8_t *status /* ncams or NULL */, double *cost /* 2 ncams: before, after; or NULL */,
                            int64_t *counts /* BA_PT_STATES + 1 (last: cameras flagged BEHIND) or NULL */, int *iters_max /* or NULL */);
int ba_resect_cameras_focal_dev(ba_problem *p, double *d_x_inout /* nvar, device */, int max_iter, double xtol, double lambda0,
                                uint8_t *d_status /* ncams or NULL */, double *d_cost /* 2 ncams or NULL */,
                                int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */, void *stream);
int ba_ransac_cameras_focal(ba_problem *p, double *x_inout /* nvar, host */, const ba_ransac_opts *opts, int max_iter, double xtol,
                            double lambda0, uint8_t *status /* ncams or NULL */, double *cost /* 2 ncams or NULL */,
                            int64_t *counts /* BA_PT_STATES + 1 or NULL */, int *iters_max /* or NULL */,
                            uint8_t *inlier /* nobs or NULL */, int32_t *n_inliers /* ncams or NULL */, int32_t *best_hyp /* ncams or NULL */);
int ba_ransac_cameras_focal_dev(ba_problem *p, double *d_x_inout /* nvar, device */, const ba_ransac_opts *opts /* host */,
                                int max_iter, double xtol, double lambda0, uint8_t *d_status /* ncams or NULL */,
                                double *d_cost /* 2 ncams or NULL */, int64_t *counts /* host, or NULL */,
                                int *iters_max /* host, or NULL */, uint8_t *d_inlier /* nobs or NULL */,
                                int32_t *d_n_inliers /* ncams or NULL */, int32_t *d_best_hyp /* ncams or NULL */, void *stream);

/* ---- relative pose of camera pairs: the eight-point essential matrix with RANSAC (an extension) ------------------------------
 * The entries above need posed cameras or placed points to start from.  This one needs neither: from the detections alone it
 * gives the pose of camera b against camera a of a pair, from the points both observe, robust against wrong matches.  With
 * compose_relative of the Python package the two cameras are posed, ba_refine_points triangulates the first points,
 * ba_ransac_cameras registers further cameras, and the LM solve refines.
 * ba_pair_matches (host only, no handle, no device): the match list of every pair (a, b), 1-based cameras.  Walk camera a's
 * observations in the caller's order: an observation of point P is a match iff it is a's first observation of P and b observes
 * P; its partner is b's first observation of P in the caller's order.  The matches of a pair are thus ordered by a's list and a
 * point gives at most one.  match_ptr receives npairs + 1 offsets; obs_a1 / obs_b1 (both or neither: with both NULL the call
 * only counts) the 1-based observations of every match.  a == b, an index out of range, a NULL array: BA_ERR_ARG; npairs == 0
 * is fine; a pair may repeat and a camera may appear in many pairs.
 * ba_relative_pose: x is a host vector of which only (k1, k2, f) of the pairs' cameras are read; its poses and points never are
 * (NaN is fine).  From the handle only ba_lm_set_obs_info is honoured, and only through the test Lambda != 0: a match is USED iff
 * both its observations are.  Loss, mask, priors and grouping are ignored.  A handle with a communicator is refused.
 * Conventions: P_a = R_a X + t_a, P_b = R_b X + t_b; the relative pose is P_b = R P_a + t with |t| = 1 (the scale cannot be
 * observed).  The BAL camera looks down -z: the ray of an undistorted measurement q is d = (q_x, q_y, -1) and a point in front
 * is P = alpha d with alpha > 0.  The epipolar constraint is d_b' E d_a = 0 with E = [t]x R.
 * The linear fit on a set of n matches:
 *  1. q_a, q_b of a match: the undistortion of ba_resect_cameras (u = pt2d / f, 8 iterations) with each camera's intrinsics.
 *     f not finite or 0 for either camera: the pair is BA_RP_DEGENERATE.
 *  2. Hartley normalisation per image: c = the mean of q, s = sqrt(2) / (the RMS distance from c), the sums taken about the first
 *     match of the set; d~ = (s (q - c), -1).  Coinciding image points or a sum that is not finite: degenerate.
 *  3. M = sum a a' (9 x 9) with a = d~_b (x) d~_a, the row-major entries of E~.
 *  4. The eigenvector of M's smallest eigenvalue by the cyclic Jacobi sweeps of ba_resect_cameras.  An eigenvalue that is not
 *     finite, or lambda_2 <= 1e-10 lambda_9: degenerate.  This is the known limit of the method: all points on a plane (or a
 *     ruled quadric through both centres), a pure rotation (no baseline), and fewer than 8 matches in general position.
 *  5. E = T_b' E~ T_a with T = [[s, 0, s c_x], [0, s, s c_y], [0, 0, 1]] (d~ = T d: the third entry of d is -1).
 *  6. The one-sided Jacobi SVD of E as in ba_resect_cameras: U and V proper rotations, the column of the smallest singular value
 *     by cross product.  The four candidates are R = U Rz(+90) V', U Rz(-90) V' (Rz turning in the plane of the two large singular
 *     directions) with t = + or - the left null direction of E, in the order (R+, t), (R+, -t), (R-, t), (R-, -t).
 *  7. Cheirality: for a candidate and a match, (alpha, beta) solve the 2 x 2 normal equations of alpha R d_a + t = beta d_b; the
 *     match is in front iff alpha > 0 and beta > 0 (a comparison with NaN fails).  The candidate with the most matches of the set
 *     in front wins, ties to the first; a best count of 0: degenerate.
 *  8. r = the rotation vector of the winner's R (the rule of ba_resect_cameras: theta < 1e-12 gives (1e-12, 0, 0)) and its t.
 *     Everything downstream uses the clean E_h = [t]x R rebuilt from (r, t).
 * Inlier test of a match under (r, t): it is used, alpha > 0, beta > 0, and its Sampson distance in pixels^2,
 *   (d_b' E_h d_a)^2 / (((E_h d_a)_1^2 + (E_h d_a)_2^2) / f_b^2 + ((E_h' d_b)_1^2 + (E_h' d_b)_2^2) / f_a^2), is <= tau^2.
 * States: BA_RP_FEW_MATCHES -- fewer than 8 used matches; BA_RP_DEGENERATE -- a focal length as in step 1, or the final fit is
 * degenerate; BA_RP_NO_CONSENSUS -- below; BA_RP_OK.  Only a pair that is BA_RP_OK has its six entries of pose written (r, then
 * t); the others keep what the caller put there.  counts[s] = pairs in state s.
 * opts == NULL: no consensus stage -- the set is every used match (inlier = used, best_hyp = -1) and the pose is the linear fit on it.
 * opts != NULL (ba_ransac_opts unchanged; the rules of ba_ransac_cameras with these ranges): threshold tau in pixels, finite and
 * > 0; hypotheses H (<= 0: 128; at most 4096); sample m (<= 0: 8; 8..16); refits (< 0: 2; at most 8); min_inliers (<= 0:
 * max(m, 8); at least 8); seed.  Sampling: exactly ba_ransac_sample(seed, h, degree = the number of matches of the pair, used, m)
 * on the pair's match list; the pair's index does not enter.  Hypothesis h = the linear fit on the m sampled matches in the order
 * of their draws; a degenerate sample is void.  Score = the inlier count over the pair's whole list; the best hypothesis has the
 * largest count, ties to the lowest h.  No valid hypothesis, or a best count < min_inliers: BA_RP_NO_CONSENSUS, the inlier bytes
 * 0, n_inliers = the best count (0 if none), best_hyp = that h or -1.  Otherwise the winner's inliers are the set M.  Refits, up
 * to `refits` times: the linear fit on M; the whole list re-scored under it gives M'; M' is adopted iff |M'| >= |M| and
 * M' != M; otherwise (also when the fit is degenerate) M stays and the pair stops.  Finish: the linear fit on the final set is
 * the returned pose; inlier = the set, n_inliers = its size.  A pair that is FEW_MATCHES or DEGENERATE by a focal length has
 * inlier bytes 0, n_inliers = 0, best_hyp = -1.
 * Outputs, each may be NULL except pose and status: match_ptr (npairs + 1 offsets into the match lists, those of
 * ba_pair_matches), inlier (one byte per match, in that order), n_inliers, best_hyp, counts.
 * No floating-point atomics and one writer per output: two calls give the same bits, and a pair's result depends on its own
 * matches, their order, the two cameras' intrinsics and the options only.  The next ba_lm_step / ba_lm_solve on the handle gives
 * the bits it gives without this call.  npairs == 0 returns BA_OK.
 * On noisy data the eight-point fit is only a start: on a narrow field of view (the generator's unit ball seen from distance
 * 5..7, 30 % wrong matches, tau = 2 px) the final set is the true one for most pairs at 0.05 px of noise and for about half of
 * them at 0.1 px, whatever the refits; the refinement behind it (the triangulation, the resections and the LM solve on the
 * seeded x) is what makes the estimate.
 * The remedy is the five-point minimal solver as the hypothesis generator: ba_relative_pose_five_point, below.
 * The non-linear refinement of the pair on its final set is ba_refine_relative_pose, further down.
 * Planar scenes and pairs without a baseline are the business of ba_homography and ba_homography_pose, further down, and the
 * choice of the initial pair that of two_view of the Python package.
 * Out of scope: unknown focal lengths; MSAC or an adaptive hypothesis count; Float32; several ranks; a device-resident entry. */
enum { BA_RP_OK = 0, BA_RP_FEW_MATCHES = 1, BA_RP_DEGENERATE = 2, BA_RP_NO_CONSENSUS = 3, BA_RP_STATES = 4 };
int ba_pair_matches(int64_t ncams, int64_t npnts, int64_t nobs, const int64_t *cam_idx1, const int64_t *pnt_idx1,
                    int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                    int64_t *match_ptr /* npairs + 1 */, int64_t *obs_a1 /* match_ptr[npairs] or NULL */,
                    int64_t *obs_b1 /* same */);
int ba_relative_pose(ba_problem *p, const double *x /* nvar, host: only (k1, k2, f) of the pairs' cameras are read */,
                     int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                     const ba_ransac_opts *opts /* NULL: no consensus stage, the linear fit on all used matches */,
                     double *pose /* 6 npairs: rotation vector r, unit translation t */, uint8_t *status /* npairs */,
                     int64_t *match_ptr /* npairs + 1, or NULL */, uint8_t *inlier /* one byte per match, or NULL */,
                     int32_t *n_inliers /* npairs or NULL */, int32_t *best_hyp /* npairs or NULL */,
                     int64_t *counts /* BA_RP_STATES or NULL */);

/* ---- the five-point essential matrix as the minimal solver of the two-view consensus stage (an extension) ----------
 * ba_relative_pose_five_point: ba_relative_pose with another hypothesis generator.  Arguments, outputs, states (FEW_MATCHES is
 * still "fewer than 8 used matches": the refits and the final fit are eight-point fits), the communicator refusal, the inlier
 * test, the winner, the refits with their adopt rule and the final linear fit are those of ba_relative_pose.  What differs:
 *   opts must not be NULL (BA_ERR_ARG, "null options"): without a consensus stage there is nothing five-point about the call.
 *   sample (<= 0: 5) must be 5; min_inliers (<= 0: 8) at least 8; threshold, hypotheses, refits and seed as above.
 *   The sample of hypothesis h is what the sampler of ba_ransac_sample gives for m = 5 on the pair's match list.
 *   Hypothesis h: every real essential matrix through the five sampled matches (ba_five_point, below) is a candidate.  A
 *   candidate goes through steps 6-8 of the linear fit above (its SVD, the four (R, t), the cheirality vote over the five
 *   matches, the rotation vector) and is scored by its inlier count over the pair's whole list.  The hypothesis is the candidate
 *   with the largest count, ties to the candidate found first.  No sample, a degenerate null space, no real solution, or no
 *   candidate with a match in front: the hypothesis is void.
 * The eight-point fit on a whole inlier set is not what fails on noisy data; eight noisy matches are.  With five-point
 * hypotheses the consensus set at the generator's 0.5 px is the true one for most pairs.
 * ba_five_point: the solver alone, n independent problems, one wave each.  qa, qb: five undistorted image points per problem and
 * image, already divided by f; the ray is d = (q, -1).  E: per problem ten slots of 3 x 3 row-major matrices, the real solutions
 * first, each with |E|_F = 1, the unused slots NaN; n_sol: their number, 0..10.  The sign of a solution and the order of the
 * solutions are not specified; two calls give the same bits, and a problem's result does not depend on the others of the call.
 * The solver: the null space of the 5 x 9 system a_k = d_b (x) d_a on raw rays (no Hartley normalisation) as the eigenvectors
 * X, Y, Z, W of the four smallest eigenvalues of sum a a' (the Jacobi sweeps above); lambda_5 <= 1e-12 lambda_9 or a sum that is
 * not finite: 0 solutions.  E = x X + y Y + z Z + W; det E = 0 and 2 E E' E - tr(E E') E = 0 are ten cubics in 20 monomials;
 * Gauss-Jordan with partial pivoting on the 10 x 20 (a pivot that is 0 or not finite: 0 solutions); the 3 x 3 polynomial matrix
 * in z and its determinant of degree 10; its roots by a simultaneous complex iteration (Aberth-Ehrlich), a root being real when
 * |Im z| <= 1e-7 |z|; a real root takes two Newton steps on the real axis; x and y from the null vector of the 3 x 3 at the
 * root; then (x, y, z) takes two Gauss-Newton steps on the ten eliminated cubics (a step that is not finite is not taken): a
 * root of the degree-10 polynomial carries that polynomial's conditioning, the cubics carry the solution's own, and without
 * these steps an ill-conditioned tuple is wrong at 1e-4.  A derivative of the polynomial that vanishes at an iterate makes the
 * iteration fail: the tuple then has no solution.  The handle supplies the device, the stream and the buffers; a handle with a
 * communicator is fine.  n == 0 returns BA_OK. */
int ba_relative_pose_five_point(ba_problem *p, const double *x /* nvar, host: only (k1, k2, f) of the pairs' cameras are read */,
                                int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                                const ba_ransac_opts *opts /* not NULL */,
                                double *pose /* 6 npairs: rotation vector r, unit translation t */, uint8_t *status /* npairs */,
                                int64_t *match_ptr /* npairs + 1, or NULL */, uint8_t *inlier /* one byte per match, or NULL */,
                                int32_t *n_inliers /* npairs or NULL */, int32_t *best_hyp /* npairs or NULL */,
                                int64_t *counts /* BA_RP_STATES or NULL */);
int ba_five_point(ba_problem *p, int64_t n, const double *qa /* n x 5 x 2 */, const double *qb /* n x 5 x 2 */,
                  double *E /* n x 10 x 9 */, int32_t *n_sol /* n */);

/* ---- non-linear refinement of the relative pose on its consensus set (an extension) ---------------------------------
 * ba_refine_relative_pose: what ba_refine_points is to a point and ba_refine_cameras to a camera.  The pose ba_relative_pose*
 * returns is the eight-point fit on the final set; on 20..50 noisy inliers of a narrow field that linear fit is often not even
 * consistent with the set it is returned with.  This entry minimises, per pair and over the five degrees of freedom of
 * (R, t with |t| = 1), the robustified Sampson error over the pair's inlier set, and re-scores the pair's list under the result.
 * x, the pairs, the match lists, the rays (step 1 above), "used" (Lambda != 0 on both observations, the only thing honoured of
 * the handle) and the communicator refusal are those of ba_relative_pose.  pose_inout: (r, t) per pair, read and written; t is
 * taken as given, it is the caller's to pass a unit t.  status_in: the BA_RP_* of the pairs (NULL: all BA_RP_OK).  inlier_inout:
 * one byte per match in the order of ba_pair_matches; the set M of a pair is the USED matches among those with a byte != 0
 * (NULL: every used match, and no bytes are returned).
 * Residual of a match: e = n / sqrt(D), n = d_b' E d_a, D = ((E d_a)_1^2 + (E d_a)_2^2) / f_b^2 + ((E' d_b)_1^2 + (E' d_b)_2^2) /
 * f_a^2, E = [t]x R: the signed square root of the Sampson distance of the inlier test, in pixels.
 * Objective: F(R, t) = 1/2 sum over M of c^2 rho(e^2 / c^2), rho and c = f_scale (pixels) the losses of ba_lm_set_loss (opts.loss:
 * BA_LOSS_*).  Cheirality is not part of the objective; it stays in the inlier test.
 * Local parameters delta = (d_omega, d_tau) in R^3 x R^2: R+ = exp([d_omega]x) R; t+ = (t + B d_tau) / |t + B d_tau| with
 * B = [b1 b2], b1 = (e_i x t) / |e_i x t| for i the index of the smallest |t_i| (ties to the lowest), b2 = t x b1.  A step too
 * small to move any component of t leaves t as it is (the retraction of 0 is the identity, bit for bit).
 * Jacobian, analytic and exact: dE/d omega_j = [t]x [e_j]x R, dE/d tau_j = [b_j]x R, and de = dn / sqrt(D) - n dD / (2 D^(3/2))
 * with the derivative of D included.
 * Step: w = rho'(e^2 / c^2) per match, H = sum w J'J, g = sum w J'e (the reweighting of ba_refine_points); (H + lambda diag H)
 * delta = -g by a 5 x 5 Cholesky; a pivot that is not > 0 or a delta that is not finite is a rejection.  The trial is accepted
 * iff F+ is finite and F+ <= F; then lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.
 * States: BA_RR_CONVERGED -- an accepted step with |delta|_2 <= xtol (radians on both parts); BA_RR_STALLED -- lambda > 1e12;
 * BA_RR_MAX_ITER; BA_RR_NONFINITE -- F at the start is not finite, the pose is untouched; BA_RR_SKIPPED -- the pair's status_in
 * is not BA_RP_OK, a focal length is not finite or is 0, or M has fewer than 5 members: the pose, the inlier bytes, n_inliers and
 * n_consistent come back as the caller filled them, the cost entries are 0.
 * Options: max_iter (< 0: 50; 0 evaluates only and gives BA_RR_MAX_ITER with the pose's bits unchanged); xtol (<= 0: 1e-10);
 * lambda0 (<= 0: 1e-4); loss with f_scale finite and > 0; threshold tau in pixels, finite and > 0; rounds (< 0: 2; at most 8).
 * A value that is not finite, an unknown loss, rounds > 8, NULL options: BA_ERR_ARG.
 * Returned pose: r = the rotation vector of the final R by the rule of step 8 above, t = the final unit t; a pose that no
 * accepted step moved keeps its bits.
 * Rounds: round j = 0 .. rounds refines on the current set M from the current pose, then scores the pair's whole list under the
 * refined (r, t) with the inlier test above: M'.  If j < rounds, M' is adopted iff |M'| >= |M| and M' != M (the adopt rule of
 * the refits) and round j + 1 refines on it; otherwise the pair stops.
 * Per pair: pose_inout = the pose of the last refinement; inlier_inout = the set that refinement ran on, n_inliers its size;
 * n_consistent = |M'| under the returned pose; cost[2] = F before the first trial on the incoming set and F at the returned
 * pose on the returned set; iters = the trials summed over the rounds; state = that of the last refinement.
 * counts[s] = pairs in state s.  Every output but pose_inout and state may be NULL.
 * One 256-lane workgroup per pair runs the whole iteration of a round in one launch; rounds + 1 launches.  No atomics and one
 * writer per output: two calls give the same bits, a pair alone gives the bits it gives among many, and the next ba_lm_step /
 * ba_lm_solve on the handle gives the bits it gives without this call.  npairs == 0 returns BA_OK.
 * Out of scope: refining focal lengths or distortion with the pair; a device-resident entry; Float32; several ranks. */
enum { BA_RR_CONVERGED = 0, BA_RR_STALLED = 1, BA_RR_MAX_ITER = 2, BA_RR_NONFINITE = 3, BA_RR_SKIPPED = 4, BA_RR_STATES = 5 };
typedef struct ba_pair_refine_opts {
  int max_iter;     /* < 0: 50 */
  double xtol;      /* <= 0: 1e-10 */
  double lambda0;   /* <= 0: 1e-4 */
  int loss;         /* BA_LOSS_* */
  double f_scale;   /* c in pixels, > 0 */
  double threshold; /* tau in pixels, > 0 */
  int rounds;       /* < 0: 2; at most 8 */
} ba_pair_refine_opts;
int ba_refine_relative_pose(ba_problem *p, const double *x /* nvar, host: only (k1, k2, f) of the pairs' cameras are read */,
                            int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const ba_pair_refine_opts *opts,
                            double *pose_inout /* 6 npairs */, const uint8_t *status_in /* npairs, BA_RP_*; NULL: all OK */,
                            uint8_t *inlier_inout /* per match in ba_pair_matches order; NULL: every used match */,
                            uint8_t *state /* npairs */, double *cost /* 2 npairs */, int32_t *n_inliers, int32_t *n_consistent,
                            int32_t *iters, int64_t *counts /* BA_RR_STATES */);

/* ---- P3P minimal samples for the consensus stage of the camera resection (an extension) ------------------------------
 * ba_ransac_cameras_p3p: ba_ransac_cameras with another hypothesis generator.  Arguments, outputs, states, the communicator
 * refusal, the sampling rule, the inlier test, the winner, the refits with their adopt rule (linear resections on the set) and
 * the finish -- with its bit-for-bit contract with ba_resect_cameras under an information that drops the outliers -- are those of
 * ba_ransac_cameras.  What differs:
 *   sample (<= 0: 3) must be 3; min_inliers (<= 0: 6) at least 6: the refits and the finish are still the linear resection, which
 *   needs six.  threshold, hypotheses, refits and seed as there; NULL options are BA_ERR_ARG.
 *   The intrinsics (k1, k2, f) are read from x.  A camera whose f is not finite or is 0 has only void hypotheses and ends
 *   BA_PT_DEGENERATE.  There is no focal mode.
 *   The sample of hypothesis h is what the sampling rule above gives for m = 3 on the camera's list.  (ba_ransac_sample itself
 *   keeps refusing m < 6.)
 *   Hypothesis h: the three sampled measurements are undistorted with the camera's intrinsics (the fixed-point iteration of
 *   ba_resect_cameras on pt2d / f); every solution of ba_p3p (below) on them, in its order, is a candidate; a candidate is scored
 *   by its inlier count over the camera's whole list under (pose, k1, k2, f); the hypothesis is the candidate with the largest
 *   count, ties to the first.  Its record is that of ba_ransac_cameras.  No sample, a degenerate sample, no candidate: void.
 * A sample of three is clean with probability w^3 at inlier share w where a sample of six has w^6: at 65 % wrong matches 128
 * hypotheses of six hold no clean one, 128 of three hold several.
 * ba_p3p: the solver alone, n independent problems, one lane each.  q: three undistorted image points per problem, already
 * divided by f; X: their world points.  pose: per problem four slots of (r, t) with R X_i + t = s_i j_i, s_i > 0; the solutions
 * first, in ascending order of the root v of the quartic below, the unused slots NaN.  n_sol: their number, 0..4.  Two calls
 * give the same bits; a problem's result does not depend on the others of the call.  n == 0 returns BA_OK; the handle supplies
 * the device, the stream and the buffers, and a handle with a communicator is fine.
 * The solver: unit rays j_i = (q_i, -1) / |(q_i, -1)|; sides a = |X_2 - X_3|, b = |X_1 - X_3|, c = |X_1 - X_2| -- a side that
 * is 0 or not finite, or |(X_2 - X_1) x (X_3 - X_1)| <= 1e-12 c b: 0 solutions; ca = j_2.j_3, cb = j_1.j_3, cg = j_1.j_2.  With
 * the depths s_2 = u s_1 and s_3 = v s_1 the three cosine laws are two quadrics in u,
 *   u^2 - 2 cg u + 1 - (c^2 / b^2) w(v) = 0   and   u^2 - 2 ca v u + v^2 - (a^2 / b^2) w(v) = 0,   w(v) = v^2 - 2 cb v + 1,
 * u^2 + b_1 u + c_1 and u^2 + b_2 u + c_2 for short; their resultant (c_2 - c_1)^2 - (b_2 - b_1) (b_1 c_2 - b_2 c_1) is a quartic in
 * v (a coefficient that is not finite or a leading coefficient 0: 0 solutions).  Its roots by the simultaneous complex iteration of
 * ba_five_point at degree 4, a root being real when |Im z| <= 1e-7 |z|; a real root takes two Newton steps on the real axis.  The
 * real roots in ascending order: u = (c_2 - c_1)(v) / (b_1 - b_2)(v) -- when that denominator is 0 or the quotient is not
 * finite, the root cg +- sqrt(max(cg^2 - c_1(v), 0)) of the first quadric at which the second is smaller in magnitude (ties: +);
 * a root with v <= 0 or u <= 0 gives no solution; s_1 = b / sqrt(w(v)); (s_1, s_2, s_3) take two Newton steps on the three
 * cosine laws (a step that is not finite is not taken); Y_i = s_i j_i; on either side the orthonormal frame of (P_2 - P_1,
 * P_3 - P_1) -- e_1 along the first, e_3 along e_1 x (P_3 - P_1), e_2 = e_3 x e_1, as columns of F; R = F_cam F_world',
 * t = Y_1 - R X_1; r the rotation vector of step 7 of ba_resect_cameras.  A pose with a component that is not finite is no
 * solution.
 * Out of scope: P4Pf and other unknown-focal minimal solvers, a finish from the hypothesis's pose for sets smaller than six, MSAC
 * or LO-RANSAC scoring, an adaptive hypothesis count, an early exit of the scoring pass, Float32, several ranks. */
int ba_ransac_cameras_p3p(ba_problem *p, double *x_inout /* nvar, host */, const ba_ransac_opts *opts, int max_iter, double xtol,
                          double lambda0, uint8_t *status /* ncams or NULL */, double *cost /* 2 ncams or NULL */,
                          int64_t *counts /* BA_PT_STATES + 1 or NULL */, int *iters_max /* or NULL */,
                          uint8_t *inlier /* nobs or NULL */, int32_t *n_inliers /* ncams or NULL */, int32_t *best_hyp /* ncams or NULL */);
int ba_ransac_cameras_p3p_dev(ba_problem *p, double *d_x_inout /* nvar, device */, const ba_ransac_opts *opts /* host */, int max_iter,
                              double xtol, double lambda0, uint8_t *d_status /* ncams or NULL */, double *d_cost /* 2 ncams or NULL */,
                              int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */,
                              uint8_t *d_inlier /* nobs or NULL */, int32_t *d_n_inliers /* ncams or NULL */,
                              int32_t *d_best_hyp /* ncams or NULL */, void *stream);
int ba_p3p(ba_problem *p, int64_t n, const double *q /* n x 3 x 2 */, const double *X /* n x 3 x 3 */,
           double *pose /* n x 4 x 6 */, int32_t *n_sol /* n */);

/* ---- outlier-robust triangulation: RANSAC before the linear point (an extension) -----------------------------------
 * ba_refine_points with init = 1 and a consensus stage in front.  The linear triangulation sums (I - dd') over every used
 * observation of a point, unweighted: one wrong match in a track moves the point arbitrarily, the robust loss of the refinement
 * then starts from that point, and a camera registered next by ba_ransac_cameras is scored against it.  Here every point's
 * two-view hypotheses are triangulated and scored on the device, the best one defines the point's inlier set, and the
 * triangulation and the Marquardt refinement run on that set only.  The inlier mask comes back to the caller.
 * Options (ba_ransac_opts): threshold tau in pixels, finite and > 0; hypotheses H (<= 0: 128; at most 4096); sample (<= 0: 2;
 * anything else but 2 is refused); refits (< 0: 2; at most 8); min_inliers (<= 0: 2; at least 2 -- a caller who wants a third
 * view to confirm a point asks for 3); seed.  Anything else is BA_ERR_ARG, as are NULL options.  The other refusals are those of
 * ba_refine_points; as there, no communicator is needed and a shard works on its own points.
 * Which points: a point fixed by ba_lm_set_fixed is BA_PT_FIXED and not attempted: inlier = its used observations, n_inliers =
 * their number, best_hyp = -1.  Every other point is attempted; its entries in x are never read (NaN is fine).  "Used" means
 * Lambda != 0 under ba_lm_set_obs_info; the information plays no other part in the consensus stage, and point priors play none:
 * they act in the finish.
 * Hypotheses of a point: its list is its observations in the caller's order, its degree d counts the unused entries too, and
 * n = d (d - 1) / 2.
 *   n <= H: the enumeration is exhaustive.  Hypothesis h < n is the pair (a, b) of list positions, a < b, of rank h in the order
 *   (0,1), (0,2), ..., (0,d-1), (1,2), ...; a hypothesis with h >= n is void, a pair with an unused member is void; the seed is
 *   not read.
 *   n > H: the sampling of ba_ransac_cameras with m = 2 on the point's list -- the same key, the same draws, the same skip rule
 *   and the same limit of 64 draws.  The point index does not enter.
 *   The point of a hypothesis is the linear triangulation of ba_refine_points, step for step, on those two observations.  A
 *   pivot <= 1e-12 trace or a result that is not finite makes the hypothesis void.
 * Inlier test: under a point X, observation o is an inlier iff it is used, P1.z < 0 under its camera of x, and
 * |project - pt2d|^2 <= tau^2 in raw pixels with the model's own projection.  A comparison with NaN fails.
 * Selection: the score of a hypothesis is its inlier count over the point's whole list; the best is the largest count, ties to
 * the lowest h.  Without a valid hypothesis, or with a best count < min_inliers, the point fails: its inlier bytes are 0,
 * n_inliers = the best count (0 if none), best_hyp = that h or -1, state BA_PT_DEGENERATE, bit-unchanged, cost entries 0, no flag.
 * Refits, up to `refits` times: the linear triangulation on the current set M; the whole list re-scored under that point gives
 * M'; M' is adopted iff |M'| >= |M| and M' != M; otherwise (smaller, equal, or the refit was degenerate) M stays and the point
 * stops.
 * Finish: ba_refine_points(init = 1) with the observations outside the final set treated exactly as Lambda = 0 -- the linear
 * triangulation on the set, then the Marquardt refinement on the set under the handle's loss, information and point priors; an
 * outlier raises no BEHIND flag; max_iter == 0 returns the linear triangulation on the set; states, costs, counts and iters_max
 * as in that entry.  x, status and cost equal, bit for bit, those of ba_refine_points(init = 1) on the same handle whose
 * information is the caller's with the outliers' entries set to 0 (the identity on the inliers when the caller set none).
 * Outputs beyond those of ba_refine_points, each may be NULL: inlier (nobs bytes 0 / 1, caller's observation order), n_inliers
 * (npnts: the size of the final set) and best_hyp (npnts).  In the _dev form they are device pointers and the call is enqueued
 * on `stream`; it synchronises only to hand over counts / iters_max, as its sibling does.
 * Two calls give the same bits (no floating-point atomics); the next ba_lm_step / ba_lm_solve on the handle gives the same bits
 * as without the call; a point's result depends on its own list, the cameras and the options only; the camera part of x comes
 * back bit-identical.
 * Out of scope: an adaptive hypothesis count, MSAC scoring, a minimum triangulation angle, Float32, several ranks. */
int ba_ransac_points(ba_problem *p, double *x_inout /* nvar, host */, const ba_ransac_opts *opts, int max_iter, double xtol,
                     double lambda0, uint8_t *status /* npnts or NULL */, double *cost /* 2 npnts or NULL */,
                     int64_t *counts /* BA_PT_STATES + 1 or NULL */, int *iters_max /* or NULL */,
                     uint8_t *inlier /* nobs or NULL */, int32_t *n_inliers /* npnts or NULL */, int32_t *best_hyp /* npnts or NULL */);
int ba_ransac_points_dev(ba_problem *p, double *d_x_inout /* nvar, device */, const ba_ransac_opts *opts /* host */, int max_iter,
                         double xtol, double lambda0, uint8_t *d_status /* npnts or NULL */, double *d_cost /* 2 npnts or NULL */,
                         int64_t *counts /* host, or NULL */, int *iters_max /* host, or NULL */,
                         uint8_t *d_inlier /* nobs or NULL */, int32_t *d_n_inliers /* npnts or NULL */,
                         int32_t *d_best_hyp /* npnts or NULL */, void *stream);

/* ---- homography of camera pairs: consensus, decomposition and the pose of a planar pair (an extension) ---------------
 * The final fit of ba_relative_pose* is the eight-point fit, which is degenerate on the points of one plane and arbitrary on noisy
 * ones, and a pair without a baseline (a camera turned on the spot) passes the essential-matrix consensus with a meaningless t.
 * The second two-view model covers both: for matches on a plane n' P_a = d (n the unit normal in camera a's frame, d > 0 the
 * distance of camera a's centre) the rays obey d_b ~ H d_a with H = R + t n' / d, and with t = 0 every match does.
 * ba_homography: the arguments, the match lists, "used" (Lambda != 0 on both observations), the rays (step 1 of ba_relative_pose:
 * q_a, q_b, d = (q, -1); a focal length that is not finite or 0: BA_HG_DEGENERATE), the communicator refusal, the optional outputs,
 * npairs == 0 and the guarantees (no atomics, one writer per output, two calls give the same bits, a pair alone gives the bits it
 * gives among many, the next ba_lm_step / ba_lm_solve gives the bits it gives without the call) are those of ba_relative_pose.
 * States: BA_HG_FEW_MATCHES -- fewer than 4 used matches; BA_HG_DEGENERATE -- a focal length, or the final fit is degenerate;
 * BA_HG_NO_CONSENSUS; BA_HG_OK.  Only a pair that is BA_HG_OK has its nine entries of H written (row-major); the others keep
 * what the caller put there.
 * The linear fit on a set of n >= 4 matches:
 *  1. Hartley normalisation per image, exactly steps 1-2 of ba_relative_pose: the sums about the first match of the set,
 *     d~ = T d = (s (q - c), -1).  Coinciding image points or a sum that is not finite: degenerate.
 *  2. M = sum A'A (9 x 9, 45 packed sums) with A = [d~_b]x (x) d~_a' (3 x 9), the three rows of d~_b x (H~ d~_a) = 0 in the
 *     row-major entries of H~; A'A = (|d~_b|^2 I - d~_b d~_b') (x) (d~_a d~_a') is what is summed.
 *  3. H~ = the eigenvector of M's smallest eigenvalue by the cyclic Jacobi sweeps of ba_resect_cameras.  An eigenvalue that is not
 *     finite, or lambda_2 <= 1e-10 lambda_9: degenerate (three of four sampled points on a line, among others).
 *  4. H = T_b^-1 H~ T_a with T = [[s, 0, s c_x], [0, s, s c_y], [0, 0, 1]]; its singular values by the one-sided 3 x 3 Jacobi SVD
 *     of ba_resect_cameras.  sigma_3 <= 1e-6 sigma_1, or one that is not finite: degenerate.  H is divided by sigma_2.
 *  5. The sign: H is negated iff fewer than half of the set have d_b' H d_a > 0 (a comparison with NaN counts as not positive)
 *     or, at exactly half, det H < 0: a tie goes to the sign of a homography with both centres on one side of the plane, never to
 *     the arbitrary sign of the eigenvector.
 * Inlier test of a match under H: it is used; m = H d_a has m_3 < 0 and m' = adj(H) d_b has m'_3 < 0 (the adjugate: no division,
 * and the ratios below need no scale); both transfer errors in pixels^2, f_b^2 |q_b + m_1:2 / m_3|^2 and
 * f_a^2 |q_a + m'_1:2 / m'_3|^2, are <= tau^2.  A comparison with NaN fails.
 * opts == NULL: no consensus stage -- the set is every used match (inlier = used, best_hyp = -1), H the linear fit on it.
 * opts != NULL: the consensus stage of ba_relative_pose in everything but the ranges -- sample m (<= 0: 4; 4..16); min_inliers
 * (<= 0: 8; at least 4); threshold, hypotheses (<= 4096), refits (<= 8) and seed as there.  Sampling is exactly
 * ba_ransac_sample(seed, h, degree, used, m) on the pair's list (the rule: that host entry itself takes m >= 6 only).
 * Hypothesis h = the linear fit on the m sampled matches, a degenerate sample is void; score = the inlier count over the whole
 * list; the winner (ties to the lowest h), BA_HG_NO_CONSENSUS (its inlier bytes, n_inliers and best_hyp), the refits with the
 * adopt rule (M' adopted iff |M'| >= |M| and M' != M) and the finish are as there: the fit on the final set is the returned H.
 * ba_decompose_homography: the solver alone, n independent problems, one lane each, in registers.  The sign of H is taken as
 * given (ba_homography returns the sign under which the points are in front).  SVD of H by the one-sided Jacobi sweeps, sigma_1
 * >= sigma_2 >= sigma_3, H V = U Sigma; v_1 and v_3 are signed so that their entry of the largest magnitude is positive (ties to
 * the lowest index) and v_2 = v_3 x v_1, so V is proper.  An entry or a singular value that is not finite, or sigma_2 = 0:
 * n_sol = 0.  H is divided by sigma_2; parallax = sigma_1 - sigma_3, which is |t| / d for H = R + t n' / d.
 * sigma_1^2 - sigma_3^2 <= 1e-12: n_sol = 1, the rotation-only case -- R = [H v_1 / sigma_1, H v_2, their cross product] V', the
 * nearest rotation of H, t = 0, normal = 0.  Otherwise n_sol = 4, the solutions of Ma, Soatto, Kosecka and Sastry (An Invitation
 * to 3-D Vision, Alg. 5.2): u+- = (sqrt(1 - sigma_3^2) v_1 +- sqrt(sigma_1^2 - 1) v_3) / sqrt(sigma_1^2 - sigma_3^2) (a negative
 * radicand is taken as 0), U = [v_2, u, v_2 x u], W = [H v_2, H u, H v_2 x H u], R = W U', n = v_2 x u, t = (H - R) n in units of
 * d; each comes with (R, -t, -n); the order is (+), -(+), (-), -(-).  The unused slots are NaN.
 * ba_homography_pose: the pose of a planar pair.  For every pair that is BA_HG_OK in status_in (NULL: all) H is decomposed; of the
 * four solutions those whose normal has n' d_a > 0 for more than half of the set (the inlier bytes of ba_homography: the plane
 * is in front of camera a) are kept in solver order, at most two.  Per kept candidate: r by the rotation-vector rule of
 * ba_resect_cameras, t / |t|, the normal, and support = the count of the inlier test of ba_relative_pose (Sampson <= tau^2 with
 * tau = threshold, both depths > 0) over the pair's WHOLE list under that pose: the matches off the plane tell the two
 * candidates apart, and on a pure plane the counts tie.  The rotation-only case returns n_pose = 1: r is valid, t and the normal are
 * NaN and support is -1.  Every other pair: n_pose = 0, parallax NaN.  Unused entries of pose and normal are NaN, of support -1.
 * normal and support may be NULL.
 * Out of scope: a non-linear refinement of H; the choice between the two planar candidates without off-plane matches; MSAC;
 * Float32; several ranks; a device-resident entry.  The choice of the initial pair is two_view of the Python package. */
enum { BA_HG_OK = 0, BA_HG_FEW_MATCHES = 1, BA_HG_DEGENERATE = 2, BA_HG_NO_CONSENSUS = 3, BA_HG_STATES = 4 };
int ba_homography(ba_problem *p, const double *x /* nvar, host: only (k1, k2, f) of the pairs' cameras are read */,
                  int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                  const ba_ransac_opts *opts /* NULL: the linear fit on all used matches */,
                  double *H /* 9 npairs, row-major */, uint8_t *status /* npairs */,
                  int64_t *match_ptr /* npairs + 1, or NULL */, uint8_t *inlier /* one byte per match, or NULL */,
                  int32_t *n_inliers /* npairs or NULL */, int32_t *best_hyp /* npairs or NULL */,
                  int64_t *counts /* BA_HG_STATES or NULL */);
int ba_decompose_homography(ba_problem *p, int64_t n, const double *H /* n x 9 */, double *R /* n x 4 x 9 */,
                            double *t /* n x 4 x 3, in units of the plane distance */, double *normal /* n x 4 x 3 */,
                            int32_t *n_sol /* n: 0, 1 or 4 */, double *parallax /* n */);
int ba_homography_pose(ba_problem *p, const double *x /* nvar, host: only (k1, k2, f) of the pairs' cameras are read */,
                       int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const double *H /* 9 npairs */,
                       const uint8_t *status_in /* npairs or NULL */, const uint8_t *inlier /* the set of H, one byte per match */,
                       double threshold, double *parallax /* npairs */, int32_t *n_pose /* npairs: 0..2 */,
                       double *pose /* npairs x 2 x 6: r, unit t */, double *normal /* npairs x 2 x 3 or NULL */,
                       int32_t *support /* npairs x 2 or NULL */);

/* ---- rotation averaging over the view graph (an extension) -----------------------------------------------------------
 * A view graph is a list of camera pairs with a relative rotation each, some of them wrong.  Pair k is (a, b), 1-based cameras;
 * r_rel[k] is the rotation vector of R_k with R_b = R_k R_a, the r that ba_relative_pose* return.  R_{i->j} is R_k where the pair
 * is listed as (i, j) and R_k' where it is listed as (j, i).  All angles are radians.  The angle of a rotation matrix M is
 * atan2(|w| / 2, (tr M - 1) / 2), w its skew part (the rule of ba_resect_cameras' rotation vector).  Every entry refuses, on the
 * host and before any device call (BA_ERR_ARG): a camera outside 1..ncams, a pair of one camera, a pair of cameras listed twice
 * in either orientation.  used: one byte per pair or NULL (all); a pair whose r_rel is not finite is never used.
 * ba_rotation_loops: for every used pair k = (a, b) and every camera c for which (a, c) and (b, c) are both used pairs,
 * L = R_{c->a} R_{b->c} R_{a->b}; n_loops[k] counts these triangles and support[k] those with angle L <= threshold (finite, > 0).
 * An unused pair gets 0, 0.  One wave per pair over a CSR adjacency sorted by neighbour; integer counts, no atomics.
 * ba_view_graph_forest: host only, no handle, no device.  The maximum spanning forest of the used pairs under the total order
 * support descending (NULL: all equal), weight descending (NULL: all 1; finite, >= 0), pair index ascending -- unique under that
 * order.  component[c]: the components numbered 0, 1, .. in the order of their lowest camera, -1 for a camera without a used
 * pair.  The root of a component: its lowest fixed camera (fixed: one byte per camera or NULL) where it has one, else the camera
 * with the largest sum of the weights of its used pairs (summed in pair order), ties to the lowest index.  parent_pair[c]: the
 * 0-based pair that joins c to its parent, -1 for roots and cameras outside the graph.  order (n_order entries, 1-based): the
 * cameras breadth first from the roots, component after component, the neighbours of a camera in ascending order.  roots
 * (n_components entries, 1-based).
 * ba_average_rotations: the absolute rotation of every camera from all pairs at once, R_b ~ R_k R_a.
 *  1. kept = used.  With opts->loops != 0: ba_rotation_loops at opts->loop_threshold first; a used pair with n_loops > 0 and
 *     support < min_support (<= 0: 1) is dropped; a pair without a triangle cannot be checked and is kept.
 *  2. The forest of the kept pairs (key: the support with loops, else the weight alone; the fixed cameras).
 *  3. Start: r0 != NULL: Exp of r0 (finite for every camera with a used pair, else BA_ERR_ARG).  r0 == NULL: the root gets I and
 *     a child R_{parent->child} R_parent along the forest.  fixed cameras are held at r0, which is then required.
 *  4. Sweeps, simultaneous over the cameras (one wave per camera reads R_in, writes R_out).  For camera i and every kept pair e with
 *     neighbour j: P = R_{j->i} R_j, v_e = Log of P R_i', theta_e = |v_e|, omega_e = w_e rho'(theta_e^2 / c^2) with the loss of
 *     ba_lm_set_loss (c = f_scale in radians).  delta_i = sum omega_e v_e / sum omega_e, R_i <- Exp of (damping delta_i) times R_i; a
 *     fixed camera, or one with sum omega = 0 (or NaN), keeps its R.  Log is theta w / |w| with the branch near pi of the
 *     rotation-vector rule and 0 for theta < 1e-12; Exp is Rodrigues, I at 0.  The sums are taken in a fixed order.
 *     delta[s] = the largest |damping delta_i| of sweep s.  damping in (0, 1] (0: 0.8): below 1 it removes the eigenvalue -1 that
 *     a bipartite graph gives the simultaneous update.
 *  5. The host launches batches of min(8, remaining) sweeps and reads their delta; it stops after the first batch that holds a
 *     sweep with delta <= xtol (xtol <= 0: exactly max_sweeps sweeps; max_sweeps <= 0: 1000, at most 100000).  The result is the
 *     state after that whole batch; *sweeps is their number, delta holds that many values (room for max_sweeps, or NULL).
 *  6. The gauge is free during the sweeps.  Afterwards every component without a fixed camera is multiplied on the right by
 *     R_root' R_root,start: its root returns to its start.  The rotations of two components are unrelated.
 *  7. residual[k] = the angle of R_k R_a R_b' for every pair with a finite r_rel whose cameras lie in one component, else NaN (a
 *     dropped pair can be re-admitted by it); edge_weight[k] = rho' on a kept pair, else 0.  cost[0] at the start and cost[1] at
 *     the result: the sum over the kept pairs of w c^2 rho(theta^2 / c^2) / 2.  r (3 per camera) by the rotation-vector rule
 *     ((1e-12, 0, 0) for the identity), NaN for a camera outside the graph.
 * status: BA_RA_ISOLATED -- no kept pair; BA_RA_FIXED -- held at r0 (the root of its component or not); BA_RA_ROOT -- the
 * root of a component without a fixed camera; BA_RA_OK.  counts: cameras per state.  n_loops and support (NULL, or npairs: 0 without loops).
 * Deterministic: two calls give the same bits; the maximum of a sweep is an unsigned 64-bit atomic maximum on the bits of a
 * non-negative double, which does not depend on the order.  The next ba_lm_step / ba_lm_solve gives the bits it gives without
 * the call.  A simultaneous update needs sweeps growing with the square of the graph's diameter.
 * Out of scope: translation averaging, camera centres, a linear solve of the step, Float32, several ranks. */
enum { BA_RA_OK = 0, BA_RA_ROOT = 1, BA_RA_FIXED = 2, BA_RA_ISOLATED = 3, BA_RA_STATES = 4 };
typedef struct ba_rotavg_opts {
  int loss;              /* BA_LOSS_* */
  int max_sweeps;        /* <= 0: 1000; at most 100000 */
  int loops;             /* != 0: the loop filter of step 1 */
  int min_support;       /* <= 0: 1 */
  double f_scale;        /* c, radians; finite and > 0 unless the loss is linear */
  double damping;        /* (0, 1]; 0: 0.8 */
  double xtol;           /* radians; <= 0: exactly max_sweeps sweeps */
  double loop_threshold; /* radians; finite and > 0 with loops */
} ba_rotavg_opts;
int ba_rotation_loops(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                      const double *r_rel /* 3 npairs */, const uint8_t *used /* npairs or NULL */, double threshold,
                      int32_t *n_loops /* npairs */, int32_t *support /* npairs */);
int ba_view_graph_forest(int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                         const uint8_t *used /* npairs or NULL */, const int32_t *support /* npairs or NULL */,
                         const double *weights /* npairs or NULL */, const uint8_t *fixed /* ncams or NULL */,
                         int32_t *component /* ncams */, int64_t *parent_pair /* ncams */, int64_t *order /* ncams */,
                         int64_t *n_order, int64_t *n_components, int64_t *roots /* ncams */);
int ba_average_rotations(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                         const double *r_rel /* 3 npairs */, const double *weights /* npairs or NULL */,
                         const uint8_t *used /* npairs or NULL */, const double *r0 /* 3 ncams or NULL */,
                         const uint8_t *fixed /* ncams or NULL */, const ba_rotavg_opts *opts, double *r /* 3 ncams */,
                         uint8_t *status /* ncams */, int32_t *component /* ncams */, uint8_t *kept /* npairs */,
                         int32_t *n_loops /* npairs or NULL */, int32_t *support /* npairs or NULL */,
                         double *residual /* npairs */, double *edge_weight /* npairs */, int32_t *sweeps,
                         double *delta /* max_sweeps or NULL */, double *cost /* 2 or NULL */,
                         int64_t *counts /* BA_RA_STATES or NULL */);

/* ---- translation averaging over the view graph (an extension) --------------------------------------------------------
 * Camera centres from the baseline directions of the pairs.  Pair k is (a, b), 1-based cameras; dir[k] (3 per pair) is the
 * direction of the baseline in the world frame, d_k ~ (C_b - C_a) / |C_b - C_a|: -R_b' t_k with the unit t of ba_relative_pose*
 * (P_b = R P_a + t) and the R_b of ba_average_rotations.  dir need not be normalised: d = dir / sqrt((x x + y y) + z z) on the
 * device.  The direction from i to j is d_k where the pair is listed as (i, j) and -d_k where it is listed as (j, i).  Angles are
 * radians; the angle between two vectors is atan2(|x cross y|, x . y).  Every entry refuses, on the host and before any device
 * call (BA_ERR_ARG), what the rotation section refuses: a camera outside 1..ncams, a pair of one camera, a pair of cameras listed
 * twice in either orientation.  used: one byte per pair or NULL (all); a pair whose dir is not finite or has a norm < 1e-12 is
 * never used.
 * ba_translation_loops: for every used pair k = (a, b) and every camera c for which (a, c) and (c, b) are both used pairs, with
 * d1 the direction a -> c and d2 the direction c -> b, d_k lies in the plane of the triangle between the two: e = the angular
 * distance of d_k to the shorter great-circle arc from d1 to d2.  n = d1 cross d2.  |n| < 1e-6 and d1 . d2 > 0: the arc is the
 * point d1, e = the angle between d_k and d1.  |n| < 1e-6 and d1 . d2 <= 0: the triangle cannot be checked and is not counted.
 * Otherwise n^ = n / |n|, q = d_k - (d_k . n^) n^; if (d1 cross q) . n^ >= 0 and (q cross d2) . n^ >= 0 then
 * e = asin min(1, |d_k . n^|), else e = min(angle(d_k, d1), angle(d_k, d2)).  n_loops[k] counts the checked triangles,
 * support[k] those with e <= threshold (finite, > 0).  An unused pair gets 0, 0.  One wave per pair over a CSR adjacency sorted
 * by neighbour; integer counts, no atomics.
 * ba_average_translations: the centre of every camera from all pairs at once, up to the gauge (a shift and a scale per
 * component).
 *  1. kept = used.  With opts->loops != 0: ba_translation_loops at opts->loop_threshold first; a used pair with n_loops > 0 is
 *     dropped if support < min_support (<= 0: 1) or if (double)support < min_ratio * (double)n_loops -- one IEEE double product
 *     and one comparison of doubles; min_ratio in [0, 1], 0: off.  A pair without a checked triangle is kept.
 *  2. The forest of the kept pairs by the rules of ba_view_graph_forest (key: the support with loops, else the weight alone;
 *     the fixed cameras).
 *  3. Start: c0 != NULL: c0 (finite for every camera with a used pair, else BA_ERR_ARG).  c0 == NULL: the root at 0 and
 *     child = parent + the direction parent -> child along the forest, so every tree baseline has length 1.  fixed cameras are held
 *     at c0, which is then required.
 *  4. Cost: F(c) = sum over the kept pairs of w_k c^2 rho(|u^_k - d_k|^2 / c^2) / 2, u_k = c_b - c_a, u^ = u / |u|, rho the loss
 *     of ba_lm_set_loss with c = f_scale in units of the chord (about radians for small angles).  A kept pair with |u_k| < 1e-12
 *     has no direction: it adds w_k c^2 rho(4 / c^2) / 2 to the cost and nothing to the linearisation of that iteration.
 *  5. Linearisation: r_k = u^_k - d_k, omega_k = w_k rho', A_k = (omega_k / |u_k|^2)(I - u^ u^'), g_k = (omega_k / |u_k|)(I - u^ u^') r_k.
 *     Camera i: g_i = the sum of -g_k over the pairs it is first in and +g_k over those it is second in, D_i = the sum of A_k.
 *     The system is (H + lambda diag H) delta = -g, H delta at camera i = sum A_k (delta_i - delta_j); a fixed camera has
 *     delta = 0.  Preconditioner: the inverse (by cofactors) of D_i + lambda diag D_i.  A block with det <= 1e-12 tr^3 is
 *     singular (fewer than two edges that are not parallel and no damping on some axis): that camera has delta_i = 0 in this solve.
 *  6. Preconditioned conjugate gradients from delta = 0, on the device: one wave per camera for the product, per-camera terms
 *     of the dot products summed in camera order by one workgroup; alpha, beta and |r|_M = sqrt(r' M r) stay on the device.  The
 *     iteration after which |r|_M <= cg_tol |r0|_M (or is NaN) is the last; so is one with p' H p <= 0, whose step is not taken;
 *     g = 0 takes no iteration.  The host launches batches of min(16, remaining) iterations and reads the stop flag and the
 *     count after each; the iterations of a batch after the last are no-ops, so the result does not depend on the batch.  At
 *     most max_cg iterations (<= 0: 500; at most 100000).
 *  7. Levenberg-Marquardt on the host (ba_transavg_lm_decide, host only, is the rule): lambda starts at lambda0 (<= 0: 1e-3).  The
 *     trial c + delta is accepted iff F(trial) < F; then lambda <- max(lambda / 3, 1e-9), else lambda <- 4 lambda.  The solve
 *     stops after the iteration at which, the first that holds, |F - F(trial)| <= ftol F (<= 0: 1e-10; stop 1), the new
 *     lambda > 1e8 (stop 2), or max_iterations (<= 0: 50; at most 100000) are done (stop 3).  trace: one row of four per iteration:
 *     F(trial), the lambda of the solve, its conjugate-gradient iterations, accepted (room for 4 max_iterations, or NULL).
 *  8. Gauge: a component with a fixed camera is left as solved.  A component without one is moved so that its root is back at
 *     its start and scaled about the root so that the mean length of its kept baselines is that of the start (host arithmetic,
 *     sums in pair order).  The centres of two components are unrelated.
 *  9. residual[k] = the angle between u^_k and d_k for every pair with a usable dir whose cameras lie in one component (NaN else,
 *     and for |u_k| < 1e-12); edge_weight[k] = rho' on a kept pair, else 0; cost[0] = F at the start, cost[1] at the result; c (3
 *     per camera) is NaN for a camera outside the graph; status, component and counts as in ba_average_rotations (BA_TA_* =
 *     BA_RA_*).  n_loops and support: NULL, or npairs (0 without loops).
 * Deterministic: two calls give the same bits.  The next ba_lm_step / ba_lm_solve gives the bits it gives without the call.
 * Out of scope: a 1DSfM-style 1-D filter of the pairs, pairwise baseline lengths, Float32, several ranks, moving the sweeps of
 * ba_average_rotations onto the conjugate gradient. */
enum { BA_TA_OK = 0, BA_TA_ROOT = 1, BA_TA_FIXED = 2, BA_TA_ISOLATED = 3, BA_TA_STATES = 4 };
typedef struct ba_transavg_opts {
  int loss;              /* BA_LOSS_* */
  int loops;             /* != 0: the loop filter of step 1 */
  int min_support;       /* <= 0: 1 */
  int max_iterations;    /* <= 0: 50; at most 100000 */
  int max_cg;            /* <= 0: 500; at most 100000 */
  double f_scale;        /* c, chordal units; finite and > 0 unless the loss is linear */
  double loop_threshold; /* radians; finite and > 0 with loops */
  double min_ratio;      /* [0, 1]; 0: off */
  double ftol;           /* <= 0: 1e-10 */
  double cg_tol;         /* <= 0: 1e-6 */
  double lambda0;        /* <= 0: 1e-3 */
} ba_transavg_opts;
int ba_translation_loops(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                         const double *dir /* 3 npairs */, const uint8_t *used /* npairs or NULL */, double threshold,
                         int32_t *n_loops /* npairs */, int32_t *support /* npairs */);
int ba_average_translations(ba_problem *p, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1,
                            const double *dir /* 3 npairs */, const double *weights /* npairs or NULL */,
                            const uint8_t *used /* npairs or NULL */, const double *c0 /* 3 ncams or NULL */,
                            const uint8_t *fixed /* ncams or NULL */, const ba_transavg_opts *opts, double *c /* 3 ncams */,
                            uint8_t *status /* ncams */, int32_t *component /* ncams */, uint8_t *kept /* npairs */,
                            int32_t *n_loops /* npairs or NULL */, int32_t *support /* npairs or NULL */,
                            double *residual /* npairs */, double *edge_weight /* npairs */, int32_t *iterations,
                            int32_t *cg_iterations, double *trace /* 4 max_iterations or NULL */, double *cost /* 2 or NULL */,
                            int64_t *counts /* BA_TA_STATES or NULL */);
/* The rule of step 7, host only: returns accepted (0 / 1); *lambda_next and *stop (0, or 1..3 as above) may be NULL. */
int ba_transavg_lm_decide(double F, double F_trial, double lambda, int iteration /* 1-based */, int max_iterations, double ftol,
                          double *lambda_next, int *stop);

/* ---- similarity alignment of reconstructions: scale, rotation, shift with RANSAC (an extension) ----------------------
 * Every product of the front end lives in a frame of its own: ba_average_translations returns centres up to a shift and a scale
 * per component, a seeded reconstruction has a baseline of 1, and the priors of ba_lm_set_priors (ground control, GPS, an earlier
 * solve) live in the caller's frame.  ba_similarity brings one into the other from 3D-3D correspondences, some of them wrong.
 * Problem k owns the rows row_ptr[k] .. row_ptr[k + 1] (0-based, row_ptr[0] = 0, not decreasing), n = row_ptr[nprob], and asks
 * for (s, R, t) with dst ~ s R src + t: many problems in one call merge sub-models or the components of a view graph, one problem
 * is georeferencing.  The handle supplies the device, the stream and the buffers, as for ba_decompose_homography: no model data
 * is read.  A handle with a communicator is refused, as the siblings refuse it; nprob == 0 returns 0; n >= 2^31 is BA_ERR_ARG (the
 * kernels index rows with int); a NULL p, row_ptr, sim or status, and a NULL src or dst with n > 0, are BA_ERR_ARG.
 * Used rows: a row is used iff `used` is NULL or its byte is non-zero, and all six of its numbers are finite (the cameras that
 * ba_average_translations leaves at NaN drop out this way).  Fewer than 3 used rows: BA_SM_FEW_ROWS.
 * Options (ba_ransac_opts, reused): threshold tau in the units of dst, finite and > 0; hypotheses H (<= 0: 128; at most 4096);
 * sample m (<= 0: 3; 3..16); refits (< 0: 2; at most 8); min_inliers (<= 0: max(m, 3); at least 3); seed as the siblings.
 * Anything else is BA_ERR_ARG.
 * The fit of a set M of m >= 3 rows -- the one definition for hypotheses, refits and the final fit:
 *  1. o = the first row of M: for a hypothesis the first of its draws, for a set the lowest list index.  a_k = src_k - src_o and
 *     b_k = dst_k - dst_o.
 *  2. One pass forms 16 sums: sum a (3), sum b (3), sum |a|^2 (1), sum b a' (9).
 *  3. m_a = sum a / m and m_b = sum b / m; v_a = sum |a|^2 - m |m_a|^2 and K = sum b a' - m m_b m_a'.
 *  4. K = U Sigma V' by the one-sided 3 x 3 Jacobi SVD of ba_resect_cameras (rotations of column pairs of K until they are
 *     orthogonal: K V = U Sigma, V a product of rotations).  R is the nearest proper rotation it defines: the sign goes on the
 *     smallest singular value, whose column of U is taken as the cross product of the other two (in cyclic order, so det U = +1).
 *     d = -1 where that turned the column against K V's own, else +1; R = U V'.
 *  5. s = (sigma_1 + sigma_2 + d sigma_3) / v_a when with_scale is set, else 1 (sigma_1 >= sigma_2 >= sigma_3).
 *  6. t = (dst_o + m_b) - s R (src_o + m_a).
 * Degenerate (void as a hypothesis, BA_SM_DEGENERATE as the final fit): any of the 16 sums is not finite; v_a <= 0;
 * sigma_2 <= 1e-10 sigma_1 (collinear rows) or a singular value that is not finite; s is not finite or <= 0.  Coplanar rows are
 * not degenerate.
 * Inlier test of a row under (s, R, t): it is used and |s R src + t - dst|^2 <= tau^2.  A comparison with NaN fails.
 * opts == NULL: no consensus stage -- the set is every used row (inlier = used, best_hyp = -1), the fit on it is returned.
 * opts != NULL: the consensus stage of ba_ransac_cameras.  Sampling is exactly ba_ransac_sample(seed, h, degree, used, m) on the
 * problem's list in the caller's order (the rule: that host entry itself takes m >= 6 only).  Hypothesis h = the fit on the m
 * sampled rows in the order of their draws, a degenerate sample is void; score = the inlier count over the whole list; the winner
 * is the largest count, ties to the lowest h.  Without a valid hypothesis, or with a best count < min_inliers:
 * BA_SM_NO_CONSENSUS, inlier bytes 0, n_inliers = the best count (0 if none), best_hyp = that h or -1.  Refits, up to `refits`
 * times: the fit on the current set M; the whole list re-scored under it gives M'; M' is adopted iff |M'| >= |M| and M' != M,
 * otherwise (smaller, equal, or the refit was degenerate) M stays and the problem stops.  The fit on the final set is returned.
 * Outputs: only a problem that is BA_SM_OK has its seven entries of sim written -- s, the rotation vector of R by the rule of
 * ba_resect_cameras (theta < 1e-12: (1e-12, 0, 0)), t; the others keep what the caller put there.  inlier (n bytes 0 / 1), n_inliers
 * (the size of the final set; 0 for BA_SM_FEW_ROWS), best_hyp, rms (the root mean square of |s R src + t - dst| over the final
 * set under the returned fit; NaN where the problem is not BA_SM_OK) and counts (problems per state) may each be NULL.
 * Two calls give the same bits: the sums run in a fixed order (strided partial sums per thread, the butterfly of a wave, the four
 * waves in order), there are no floating-point atomics and every output has one writer; a problem alone gives the bits it gives
 * among many; the next ba_lm_step / ba_lm_solve on the handle gives the bits it gives without the call.
 * Out of scope: per-row weights or covariances; MSAC or LO-RANSAC scoring; an adaptive hypothesis count; reflections; Float32;
 * several ranks. */
enum { BA_SM_OK = 0, BA_SM_FEW_ROWS = 1, BA_SM_DEGENERATE = 2, BA_SM_NO_CONSENSUS = 3, BA_SM_STATES = 4 };
int ba_similarity(ba_problem *p, int64_t nprob, const int64_t *row_ptr /* nprob + 1 */,
                  const double *src /* 3 n */, const double *dst /* 3 n */, const uint8_t *used /* n or NULL */,
                  const ba_ransac_opts *opts /* NULL: the fit on all used rows */, int with_scale,
                  double *sim /* 7 nprob: s, rotation vector r, t */, uint8_t *status /* nprob */,
                  uint8_t *inlier /* n or NULL */, int32_t *n_inliers /* nprob or NULL */,
                  int32_t *best_hyp /* nprob or NULL */, double *rms /* nprob or NULL */,
                  int64_t *counts /* BA_SM_STATES or NULL */);

/* What a handle holds of the reduced camera matrix, in 128 x 128 tiles of its scalar type (Float64; a Float32 factorisation
 * adds half of that again): tiles_full = the whole lower triangle, nt (nt + 1) / 2; tiles_held = what this handle allocated
 * for S; tiles_staging = the staging buffer of the chunked assembly.  One GPU (and BA_DIST_FACTOR=0): held = full,
 * staging = 0 -- unless the block-sparse list schedule is in use, which allocates the pattern's tiles only.  Distributed factorisation: a rank holds its own tile columns only (about full / world) plus a staging
 * chunk of at most half of that -- per-rank ownership of S.  Valid after the first direct solve. */
int ba_lm_schur_memory(ba_problem *p, int64_t *tiles_full, int64_t *tiles_held, int64_t *tiles_staging);

/* ---- per-kernel timing (hipEvent pairs on the handle's stream) ------------------------------------ */
int ba_profile_enable(ba_problem *p, int on);
int ba_profile_reset(ba_problem *p);
/* fills up to cap entries; returns the number of kernel classes in *n.  names[i] points into static storage. */
int ba_profile_get(ba_problem *p, int cap, const char **names, double *total_ms, int64_t *calls, int *n);

/* dense blocked LDL^T on the f64 matrix cores, exposed for tests / roofline measurement:
 * factor the symmetric n x n matrix whose lower triangle is given row-major (ld = n) in host memory and
 * solve A x = b.  status BA_ERR_ZERO_PIVOT on an exactly zero pivot. */
int ba_dense_ldl_solve(int device, int64_t n, const double *a_lower_rowmajor, const double *b, double *x,
                       double *factor_ms);
/* the same with matrix and right-hand side rounded to Float32, factored and solved in Float32 (what
 * facto_type = Float32 does to the reduced camera system; src/lm.jl:170-173 does it to the augmented matrix) */
int ba_dense_ldl_solve_f32(int device, int64_t n, const double *a_lower_rowmajor, const double *b, double *x,
                           double *factor_ms);

/* the same matrix against nrhs right-hand sides: ONE factorisation, then forward and backward sweeps that take all columns
 * through every tile of the factor together (a chain of nt launches each way, whatever nrhs is) -- what the bordered solve of
 * shared intrinsics runs on its 3G <= 24 border columns.  B and X: n x nrhs, column-major (X may be B) */
int ba_dense_ldl_solve_multi(int device, int64_t n, const double *a_lower_rowmajor, int nrhs,
                             const double *B /* n x nrhs, column-major */, double *X, double *factor_ms);

#ifdef __cplusplus
}
#endif
#endif /* BA_HIP_H */
