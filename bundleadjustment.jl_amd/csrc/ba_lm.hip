// Levenberg-Marquardt controller (host) over the device kernels.
//
// Control flow, constants and stopping tests follow the reference line by line:
//   variant 1: src/lm.jl:15-418            (lambda0 = max(lambda, 1e10/|J'r|), ared >= 1e-4 pred, line search)
//   variant 0: src/LevenbergMarquardt.jl:16-385 (what src/solve_ba.jl runs)
// What differs is how the linear step is obtained: the reference factors the augmented matrix
// K = [[I J];[J' -lambda I]] (src/lm.jl:68-100,154-238); here the residual rows and point columns of K are
// eliminated in closed form on the device (ba_normal_kernels.hip) and the remaining reduced camera system is
// factored densely on the f64 matrix cores (ba_dense_ldl.hip).  Both give (J'J + lambda I) delta = -J' r and
// 1/2|delta_r|^2 = 1/2|J delta + r|^2 (K [dr; d] = [-r; 0]  <=>  dr = -(r + J d)), which is evaluated directly.
//
// One device->host copy of a handful of scalars per iteration drives the accept/reject logic, as the reference's
// norm() calls do.  As in the reference, a rejected step only changes the damping: J, Hpp, Hcc, gp, gc are reused.
// That logic -- defaults, accept tests, damping updates, stopping tests, log row, status -- is LMController
// (ba_lm_controller.h, host only); lm_solve_impl here is the device loop that feeds it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ba_internal.h"
#include "ba_lm_controller.h"  // LMController: the scalar decisions of ba_lm_solve (host only)
#include "ba_lm_internal.h"

namespace {

double wall() {
  using namespace std::chrono;
  return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// scalar slots.  "sharded" sums are partial per rank and all-reduced; "replicated" ones are identical on every rank.
// slots 0..2 (3 under a robust loss) are refreshed (and reduced) with the linearisation, slots 4..6 with every trial step.
// Robust loss (ba_lm_set_loss): SH_RSQ and SH_RSQ_TRIAL hold 2 f = sum c^2 rho(z) instead of |r|^2, SH_RTSQ |r~|^2
enum { SH_RSQ = 0, SH_GP, SH_X_P, SH_RTSQ, SH_RSQ_TRIAL, SH_MODEL, SH_DELTA_P, SH_COUNT = 8 };
constexpr int SH_LIN_COUNT = 3, SH_TRIAL_FIRST = 4, SH_TRIAL_COUNT = 3;
enum { RP_DELTA_C = 0, RP_X_C, RP_GC, RP_COUNT = 8 };
// (an all-reduce takes the slots of one refresh as one run: the linearisation's from slot 0, SH_RTSQ right behind them)
static_assert(SH_RSQ == 0 && SH_X_P == SH_LIN_COUNT - 1 && SH_RTSQ == SH_LIN_COUNT, "linearisation slots: one run from slot 0");
static_assert(SH_RSQ_TRIAL == SH_TRIAL_FIRST && SH_DELTA_P == SH_TRIAL_FIRST + SH_TRIAL_COUNT - 1, "trial slots: one run");
static_assert(SH_RTSQ < SH_TRIAL_FIRST && SH_TRIAL_FIRST + SH_TRIAL_COUNT <= SH_COUNT, "the two runs do not overlap");

// Build the (camera_a >= camera_b)-sorted list of observation pairs sharing a point.  "Camera" here is the BLOCK ROW of S the
// camera sits at: pos[c] under a fill-reducing camera ordering (empty: c itself).
int build_tasks(ba_problem *p, SchurTasks *T, const std::vector<int> &pos) {
  const int64_t ncams = p->ncams, npnts = p->npnts;
  const std::vector<int> &ptr = p->h_pt_ptr, &obs = p->h_pt_obs;
  std::vector<int> cam_at;
  if (!pos.empty()) {
    cam_at.resize(p->h_cam0.size());
    for (size_t o = 0; o < cam_at.size(); o++) cam_at[o] = pos[(size_t)p->h_cam0[o]];
  }
  const std::vector<int> &cam = pos.empty() ? p->h_cam0 : cam_at;
  // pass 1: tasks per camera_a
  std::vector<int64_t> ca_ptr((size_t)ncams + 1, 0);
  int64_t ntasks = 0;
  for (int64_t pt = 0; pt < npnts; pt++)
    for (int qa = ptr[(size_t)pt]; qa < ptr[(size_t)pt + 1]; qa++) {
      int ca = cam[(size_t)obs[(size_t)qa]];
      for (int qb = ptr[(size_t)pt]; qb < ptr[(size_t)pt + 1]; qb++)
        if (ca >= cam[(size_t)obs[(size_t)qb]]) {
          ca_ptr[(size_t)ca + 1]++;
          ntasks++;
        }
    }
  if (ntasks > (int64_t)2000000000) {
    ba_set_error("Schur task list too long (%lld)", (long long)ntasks);
    return BA_ERR_ARG;
  }
  for (int64_t c = 0; c < ncams; c++) ca_ptr[(size_t)c + 1] += ca_ptr[(size_t)c];
  // pass 2: bucket by camera_a (point order preserved)
  std::vector<int> ta((size_t)ntasks), tb((size_t)ntasks);
  {
    std::vector<int64_t> cur(ca_ptr.begin(), ca_ptr.end() - 1);
    for (int64_t pt = 0; pt < npnts; pt++)
      for (int qa = ptr[(size_t)pt]; qa < ptr[(size_t)pt + 1]; qa++) {
        int oa = obs[(size_t)qa], ca = cam[(size_t)oa];
        for (int qb = ptr[(size_t)pt]; qb < ptr[(size_t)pt + 1]; qb++) {
          int ob = obs[(size_t)qb];
          if (ca >= cam[(size_t)ob]) {
            int64_t q = cur[(size_t)ca]++;
            ta[(size_t)q] = oa;
            tb[(size_t)q] = ob;
          }
        }
      }
  }
  // pass 3: inside each camera_a bucket, stable counting sort by camera_b; emit keys (diagonal key always)
  std::vector<int> sa((size_t)ntasks), sb((size_t)ntasks), key_ptr, key_ca, key_cb;
  std::vector<int> cnt((size_t)ncams + 1);
  key_ptr.push_back(0);
  for (int64_t ca = 0; ca < ncams; ca++) {
    const int64_t b0 = ca_ptr[(size_t)ca], b1 = ca_ptr[(size_t)ca + 1];
    std::fill(cnt.begin(), cnt.begin() + ca + 2, 0);
    for (int64_t q = b0; q < b1; q++) cnt[(size_t)cam[(size_t)tb[(size_t)q]] + 1]++;
    for (int64_t cb = 0; cb <= ca; cb++) {
      int c = cnt[(size_t)cb + 1];
      if (c > 0 || cb == ca) {
        key_ca.push_back((int)ca);
        key_cb.push_back((int)cb);
        key_ptr.push_back(key_ptr.back() + c);
      }
      cnt[(size_t)cb + 1] += cnt[(size_t)cb];
    }
    // cnt[cb] = offset of camera_b bucket inside [b0, b1)
    for (int64_t q = b0; q < b1; q++) {
      int cb = cam[(size_t)tb[(size_t)q]];
      int64_t dst = b0 + cnt[(size_t)cb]++;
      sa[(size_t)dst] = ta[(size_t)q];
      sb[(size_t)dst] = tb[(size_t)q];
    }
  }
  T->nkeys = (int64_t)key_ca.size();
  T->ntasks = ntasks;
  {  // which 128 x 128 tiles of S receive a 9 x 9 block (a block straddles at most two tile rows and two tile columns)
    const int64_t nt = std::max<int64_t>(1, (9 * ncams + NB - 1) / NB);
    T->tile_occ.assign((size_t)(nt * nt), 0);
    for (size_t q = 0; q < key_ca.size(); q++) {
      const int64_t r0 = 9 * (int64_t)key_ca[q], c0 = 9 * (int64_t)key_cb[q];
      for (int64_t ti = r0 / NB; ti <= (r0 + 8) / NB; ti++)
        for (int64_t tj = c0 / NB; tj <= (c0 + 8) / NB; tj++)
          if (ti >= tj) T->tile_occ[(size_t)(ti * nt + tj)] = 1;
    }
  }
  {  // chunking of the long keys (see SchurTasks)
    // chunk size: the partial blocks cost traffic, so as large as leaves ~8 k chunks for the chip (sweeps on MI355X: LadyBug-49
    // 4 / 8 / 16 / 32 -> 0.107 / 0.070 / 0.058 / 0.065 ms; Dubrovnik-356 8 / 32 / 128 / 256 -> 1.12 / 0.68 / 0.58 / 0.57 ms
    // (unsplit: 2.26); Venice-1778 unsplit / 8 / 32 / 128 -> 4.36 / 4.02 / 3.52 / 3.42 ms)
    int ch = 16;
    while (ch < 128 && ntasks / (2 * ch) >= 8192) ch *= 2;
    T->chunk = ch;
    std::vector<int> skey, skey_c0, ct0, ct1;
    for (int64_t k = 0; k < T->nkeys; k++) {
      const int t0 = key_ptr[(size_t)k], t1 = key_ptr[(size_t)k + 1];
      if (t1 - t0 <= 2 * ch) continue;
      skey.push_back((int)k);
      skey_c0.push_back((int)ct0.size());
      for (int t = t0; t < t1; t += ch) {
        ct0.push_back(t);
        ct1.push_back(t + ch < t1 ? t + ch : t1);
      }
    }
    skey_c0.push_back((int)ct0.size());
    T->nsplit = (int64_t)skey.size();
    T->nchunks = (int64_t)ct0.size();
    T->h_skey = skey;
    if (T->nsplit > 0) {
      BA_CHECK(upload(T->skey, skey));
      BA_CHECK(upload(T->skey_c0, skey_c0));
      BA_CHECK(upload(T->chunk_t0, ct0));
      BA_CHECK(upload(T->chunk_t1, ct1));
      BA_CHECK(T->partial.alloc(81 * T->nchunks));
    }
  }
  T->h_key_cb = key_cb;
  BA_CHECK(upload(T->key_ptr, key_ptr));
  BA_CHECK(upload(T->key_ca, key_ca));
  BA_CHECK(upload(T->key_cb, key_cb));
  BA_CHECK(upload(T->task_a, sa));
  BA_CHECK(upload(T->task_b, sb));
  return BA_OK;
}

}  // namespace

// How the linear step of a solve is obtained.  Each entry point (lm_step_impl, lm_solve_impl, ba_covariance) fills it once,
// whole, before its first launch; everything below reads it.
struct StepMode {
  int normalize = 0;       // column scaling of the camera system: 0 (:None), 1 (:J), 2 (:A)
  bool facto_f32 = false;  // the reduced camera system is factored in Float32 (never under pcg)
  bool xf32 = false;       // eltype(x) = Float32
  bool f16 = false;        // facto_type = Float16
  bool pcg = false;        // facto = PCG
  double pcg_tol = 1e-8;
  int pcg_maxit = 0;  // 0: default
};

// What a recorded sequence depends on besides the handle's buffers: the solve mode; the loss kind and scale, launch
// arguments of the robust kernels, so a sequence recorded under one loss is never replayed under another; the mask of fixed
// parameters, which decides whether (and which instantiation of) k_fix_mask is in the sequence, and its device tables,
// launch arguments too; the priors (ba_lm_set_priors): how many of each kind (which prior kernels are in the sequence, and
// their grids) and their device buffers; the per-observation information (ba_lm_set_obs_info): which instantiation of
// k_obs_scale is in the sequence, and which array it was recorded under
struct RecordedFor {
  int bits = -1;  // normalize + 4 * facto_f32 + 8 * xf32 + 16 * loss + 128 / 256 * mask tables + 512 * information (-1: nothing recorded yet)
  double loss_scale = 1.0;
  const void *d_fix_cam = nullptr, *d_fix_pnt = nullptr;
  int64_t n_pri[PRI_KINDS] = {0, 0, 0};
  const void *d_pri[PRI_KINDS][3] = {}, *d_pri_work[3] = {};
  const void *d_info = nullptr;
  int64_t info_version = 0;
  bool operator==(const RecordedFor &o) const {
    return bits == o.bits && loss_scale == o.loss_scale && d_fix_cam == o.d_fix_cam && d_fix_pnt == o.d_fix_pnt &&
           memcmp(n_pri, o.n_pri, sizeof n_pri) == 0 && memcmp(d_pri, o.d_pri, sizeof d_pri) == 0 &&
           memcmp(d_pri_work, o.d_pri_work, sizeof d_pri_work) == 0 && d_info == o.d_info && info_version == o.info_version;
  }
};
// hipGraph replay of the two launch sequences of the LM loop (launch-bound on small problems: LadyBug-49 issues ~60
// kernels of a few microseconds per iteration).  x/x_trial and r/r_trial swap on an accepted step, so each sequence
// is recorded once per parity of the swap (step, refresh); the damping reaches the recorded kernels through d_lambda.
struct RecordedSequences {
  RecordedFor made_for;
  bool off = false;  // a recording failed on this handle: plain launches from then on
  HipGraphExec step[2], refresh[2];
};

// The LM workspace of a handle (ba_problem::lm): made by lm_ensure, released by lm_free.  The recorded launch sequences are
// declared last, so they are destroyed before the buffers they reference.
struct LMWork {
  int64_t nvar = 0, nequ = 0, n = 0, npad = 0;  // n = 9*ncams
  DevBuf<double> x, x_trial, delta;
  DevBuf<double> r, r_trial, J;
  DevBuf<double> Hpp, gp, Uinv, u;
  DevBuf<double> Yobs;                   // 6/obs: U^-1 A_b' of the current damping
  bool model_done = false;               // the step's model value was formed by the back-substitution pass
  DevBuf<double> Hcc;
  // the reduce buffer and its views (lm_ensure): rhs (npad), gc (9*ncams), hdiag (npad: diag of the camera block of J'J summed over
  // all ranks, for the column scalings), scal (the SH_COUNT sharded scalars); the replicated scalars; the pinned mirrors of both
  DevBuf<double> red;
  double *rhs = nullptr, *gc = nullptr, *hdiag = nullptr, *scal = nullptr;
  DevBuf<double> scal_rep;
  PinnedBuf<double> h_sh, h_rp;
  DevBuf<double> colscale;               // nvar (normalize != None)
  // facto_type = Float16: |J_j|^2, column norms, damping vector (nvar each), quantised J (24/obs) and r; allocated on first use
  DevBuf<double> jn2, dcol, damp, Jq, rq;
  DevBuf<double> partial;                // RED_BLOCKS
  DevBuf<double> partial_multi;          // SUMSQ_JOBS x RED_BLOCKS (launch_sumsq_multi)
  DevBuf<int> cam_pnt;                   // nobs: the point of every observation in camera order (pnt0[cam_obs[q]])
  SchurTasks tasks;
  DenseLDL ldl;
  SchurChunk whole;                // a rank that holds all of S: the whole matrix as one chunk (ensure_dense)
  std::vector<SchurChunk> chunks;  // per-rank ownership of S: chunks of tile columns, assembled and reduced one by one
  DevBuf<double> stage;            // the chunk being assembled for another owner (stage_tiles tiles)
  DevBuf<float> stage32;           // its Float32 copy when the reduce travels in Float32
  int64_t stage_tiles = 0;         // (reduce-scatter assembly: all the staging tiles, stage_bufs buffers of stage_tiles / stage_bufs)
  bool assembly_rs = false;        // chunks are reduce-scattered (one segment per owner) instead of reduced onto one owner
  int stage_bufs = 1;              // 2: chunk c+1 is assembled while chunk c travels (transfer stream)
  HipEvent ev_stage_ready[2], ev_stage_free[2];
  TilePattern pattern;       // tile pattern of S after the symbolic factorisation (ensure_dense)
  bool use_pattern = false;  // the block-sparse list schedule is in use on this handle
  // fill-reducing camera ordering of the reduced camera system (`perm` of the reference's solvers, src/lm.jl:84-88): the
  // method asked for, the camera sequence it gave (block row k of S holds camera h_cam_perm[k]; empty: the caller's
  // numbering), the name of the candidate that won
  int order_method = BA_ORDER_AMD;
  std::vector<int> h_cam_perm;
  const char *order_name = "natural";
  int order_split = 0;  // the sequence eliminates from both ends: tile column pair at which the second run starts (0: one run)
  // facto_type = Float32 (src/lm.jl:170-173): Float32 copy of the reduced camera system, allocated on first use
  DenseLDLT<float> ldl32;
  DevBuf<float> rhs32;
  StepMode mode;
  // the pivot flag of the current mode's factorisation (under pcg: of its block-Jacobi preconditioner, pcg_solve)
  int *pivot_flag() const { return mode.facto_f32 ? ldl32.flag : ldl.flag; }
  // facto_type = Float16 (src/lm.jl:165-169): J_lin / r_lin / cr0: what the model value of the current step is
  // evaluated on (the Float16-rounded scaled copies in that mode, J and r otherwise), see linear_step
  // (looked up at call time: w->r / w->r_trial swap on accepted steps, a recorded graph must not pin them)
  const double *J_lin() const { return mode.f16 ? Jq : J; }
  const double *r_lin() const { return mode.f16 ? rq : r; }
  double cr0() const { return mode.f16 ? 1.0 / (0.1 * 6.55e4) : 1.0; }
  // eltype(x) = Float32 runs (BALNLPModel(file, Float32), src/BALNLPModels.jl:91): x, r and J are produced by the Float32
  // kernels and widened; every iterate is rounded to Float32.  Buffers allocated on first use.
  DevBuf<float> xf, rf, Jf;
  // the damping of the recorded sequences (RecordedSequences)
  DevBuf<double> d_lambda;   // device scalar
  PinnedBuf<double> h_lambda;  // its pinned staging
  PinnedBuf<int> h_flag;     // pinned copy of the pivot flag
  int parity = 0;
  // facto = PCG: block-Jacobi preconditioned conjugate gradients on the reduced camera system, S never formed (pcg_solve).
  // Buffers allocated on first use: iterate, residual, preconditioned residual, direction, S * direction, W U^-1 W' part
  // (n each), point-side intermediate and a zero vector (3 npnts), the 9 x 9 diagonal blocks (45 per camera).
  int64_t n_cg = 0;   // CG iterations of the current solve
  DevBuf<double> cgx, cgr, cgz, cgp, cgq, cgt;
  DevBuf<double> cgh, zero3, blk45, cg_scal;
  PinnedBuf<double> h_cg;
  DevBuf<double> rob_partial;  // 2 RED_BLOCKS: per-block partials of k_obs_scale (cost, |r~|^2)
  // shared intrinsics (ba_lm_set_shared_intrinsics).  Direct path: the grouping's tables in the order of S (grp_row:
  // the row of k1 of every member, grp_col: per row of S the column of z it belongs to or -1), made for grp_made_for =
  // ba_problem::grp_version; the border B, Y = A^-1 B and the sweeps' scratch (24 columns of npad each), the small systems.
  // :PCG: cge, the expanded direction.  All allocated on first use.
  int64_t grp_made_for = -1;
  DevBuf<int> grp_row, grp_col;
  DevBuf<double> bord_B, bord_Y, bord_w, bord_small, cge;
  RecordedSequences rec;
};

namespace {
template <typename A, typename B>
__global__ void k_convert(const A *__restrict__ in, B *__restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (B)in[i];
}
template <typename A, typename B>
int launch_convert(const A *in, B *out, int64_t n, hipStream_t st) {
  if (n <= 0) return BA_OK;
  return BA_LAUNCH((k_convert<A, B>), std::min(grid_for(n, 256), 1u << 16), 256, 0, st, in, out, n);
}
// the two directions the controller converts in, as plain functions: they take the workspace's owners as well
int launch_convert(const double *in, float *out, int64_t n, hipStream_t st) { return launch_convert<double, float>(in, out, n, st); }
int launch_convert(const float *in, double *out, int64_t n, hipStream_t st) { return launch_convert<float, double>(in, out, n, st); }
}  // namespace

// BA_DIST_FACTOR=0: keep the whole reduced camera system on every rank (one all-reduce of S, replicated factorisation)
static bool dist_factor_on(ba_problem *p) {
  static const bool off = env_off("BA_DIST_FACTOR");
  return p->comm.active() && !off;
}

static int ensure_xf32(ba_problem *p, LMWork *w) {
  if (w->xf) return BA_OK;
  BA_CHECK(w->xf.alloc(w->nvar));
  BA_CHECK(w->rf.alloc(w->nequ));
  BA_CHECK(w->Jf.alloc(24 * p->nobs));
  return BA_OK;
}

static int ensure_f32(LMWork *w) {
  if (w->rhs32) return BA_OK;  // (the last allocation: a failed call is redone whole)
  BA_CHECK(dense_ldl_alloc<float>(&w->ldl32, w->n, w->ldl.world, w->ldl.rank, false, w->ldl.own_only));
  if (w->ldl.own_only && !w->stage32) BA_CHECK(w->stage32.alloc(std::max<int64_t>(1, w->stage_tiles) * NB * NB));
  if (w->use_pattern) BA_CHECK(dense_ldl_use_pattern(&w->ldl32, &w->pattern));
  BA_CHECK(w->rhs32.alloc(w->npad));
  return BA_OK;
}

static int ensure_f16(ba_problem *p, LMWork *w) {
  if (w->Jq) return BA_OK;
  BA_CHECK(w->jn2.alloc(w->nvar));
  BA_CHECK(w->dcol.alloc(w->nvar));
  BA_CHECK(w->damp.alloc(w->nvar));
  BA_CHECK(w->Jq.alloc(24 * p->nobs));
  BA_CHECK(w->rq.alloc(w->nequ));
  return BA_OK;
}

static int lm_ensure(ba_problem *p) {
  if (p->lm) return BA_OK;
  LMWork *w = new LMWork();
  p->lm = w;
  const int64_t ncams = p->ncams, npnts = p->npnts, nobs = p->nobs;
  w->nvar = 9 * ncams + 3 * npnts;
  w->nequ = 2 * nobs;
  w->n = 9 * ncams;
  // with a communicator the tile column pairs of S are laid out by owner rank (one contiguous range per rank).  The tiles
  // themselves (n^2/2 doubles: 1 GB for Venice, 60 GB for Final-13682), the Schur task list and the per-observation Y blocks
  // are allocated by ensure_dense when a direct solve first needs them: a handle that only ever runs facto = :PCG never
  // holds anything of the size of S.
  // ... and with the distributed factorisation a rank holds ONLY its own tile columns of S (per-rank ownership): the other
  // ranks' contributions pass through a staging buffer of at most half that size, chunk by chunk (ensure_dense, linear_step)
  BA_CHECK(dense_ldl_alloc(&w->ldl, w->n, p->comm.active() ? p->comm.world : 1, p->comm.active() ? p->comm.rank : 0, true,
                           dist_factor_on(p)));
  w->npad = w->ldl.n;
  // one device buffer [rhs(npad) | gc(npad) | hdiag(npad) | SH_COUNT scalars].  gc, hdiag and the scalars refreshed with the
  // linearisation are adjacent, in this order: one all-reduce (refresh_linearisation).  (The tiles of S are their own
  // allocation, made when the first direct solve needs them: ensure_dense.)
  const int64_t red_doubles = 3 * w->npad + SH_COUNT;
  BA_CHECK(w->red.alloc(red_doubles));
  w->rhs = w->red;
  w->gc = w->rhs + w->npad;
  w->hdiag = w->gc + w->npad;
  w->scal = w->hdiag + w->npad;
  BA_HIP_CHECK(hipMemset(w->red, 0, (size_t)red_doubles * sizeof(double)));
  BA_HIP_CHECK(hipDeviceSynchronize());  // (null-stream memset: not ordered against the handle's non-blocking stream)
  BA_CHECK(w->x.alloc(w->nvar));
  BA_CHECK(w->x_trial.alloc(w->nvar));
  BA_CHECK(w->delta.alloc(w->nvar));
  BA_CHECK(w->r.alloc(w->nequ));
  BA_CHECK(w->r_trial.alloc(w->nequ));
  BA_CHECK(w->J.alloc(24 * nobs));
  BA_CHECK(w->Hpp.alloc(6 * npnts));
  BA_CHECK(w->gp.alloc(3 * npnts));
  BA_CHECK(w->Uinv.alloc(6 * npnts));
  BA_CHECK(w->u.alloc(3 * npnts));
  BA_CHECK(w->Hcc.alloc(45 * ncams));
  BA_CHECK(w->colscale.alloc(9 * ncams));
  BA_CHECK(w->partial.alloc(std::max<int64_t>(RED_BLOCKS, (npnts + 255) / 256)));  // k_wtv<true>: one partial per 256 points
  BA_CHECK(w->partial_multi.alloc((int64_t)SUMSQ_JOBS * RED_BLOCKS));
  BA_CHECK(w->rob_partial.alloc((int64_t)2 * RED_BLOCKS));
  BA_CHECK(w->cam_pnt.alloc(nobs));
  BA_CHECK(launch_cam_pnt(p, w->cam_pnt, p->stream));
  BA_CHECK(w->scal_rep.alloc(RP_COUNT));
  BA_CHECK(w->h_sh.alloc(SH_COUNT));
  BA_CHECK(w->h_rp.alloc(RP_COUNT));
  BA_CHECK(w->h_lambda.alloc(1));
  BA_CHECK(w->h_flag.alloc(1));
  BA_CHECK(w->d_lambda.alloc(1));
  return BA_OK;
}

// Per-rank ownership of S: the tile columns of every rank (one contiguous range of the owner-major layout) are cut into
// chunks of at most about half a rank's share; a chunk is assembled -- by every rank, from its own observations -- either
// straight into the owner's tiles (the owner itself) or into the staging buffer, and reduced onto the owner.  So no rank
// ever holds more of S than its own columns plus one chunk: <= 1.5 |S| / world (plus the panel buffers of the
// factorisation).  A key's 9 x 9 block can straddle two tile columns: it is listed with both chunks and each stores the
// elements that fall into its own columns (the offset table of the chunk marks the others).
static int upload_chunk_tables(LMWork *w, std::vector<std::vector<int64_t>> &cco, const std::vector<int> &col_chunk_of_col,
                               bool sparse);

// Reduce-scatter form of the chunked assembly (default; BA_ASSEMBLY=reduce keeps the chunk-onto-one-owner form).  A chunk
// reduced onto ONE owner is a many-to-one transfer: over point-to-point xGMI it moves at one link's rate.  Here a chunk is
// one slice of EVERY owner's tile columns -- `world` segments of `seg` tiles in the staging buffer, segment r a slice of rank
// r's storage (whole tile columns; shorter slices zero-padded) -- and ONE in-place reduce-scatter delivers to every owner
// its segment: all links of every GPU carry 1 / world of the chunk.  The owner then copies its segment into its tiles.  With
// two staging buffers chunk c travels on the transfer stream while chunk c+1 is assembled on the main one.  Slices per
// owner: as many as keep all staging within about half a rank's share of S (4 world with two buffers), never finer than a
// tile column; when two buffers would not fit (small problems) there is one and the transfer is in line.
// owner_cols[r]: the tile columns of rank r, ascending; col_tiles[j]: the tiles of column j (build_chunks)
static int build_chunks_rs(LMWork *w, const std::vector<std::vector<int64_t>> &owner_cols, const std::vector<int64_t> &col_tiles) {
  const DenseLDL &l = w->ldl;
  const int64_t nt = l.nt;
  const int P = l.world, me = l.rank;
  std::vector<int64_t> share((size_t)P, 0), local_off((size_t)nt, 0);
  for (int r = 0; r < P; r++) {
    int64_t run = 0;
    for (int64_t j : owner_cols[(size_t)r]) {
      local_off[(size_t)j] = run;
      run += col_tiles[(size_t)j];
    }
    share[(size_t)r] = run;
  }
  const int64_t max_share = *std::max_element(share.begin(), share.end());
  const int64_t budget = std::max<int64_t>(max_share / 2, 1);  // all staging together
  // per owner: its columns in order cut into nsl runs of about share / nsl tiles; slices[r][c] = (first column index in
  // the owner's list, one past the last); seg = the longest run
  const int nsl = 4 * P;
  std::vector<std::vector<std::pair<int64_t, int64_t>>> slices((size_t)P);
  int64_t seg = 1;
  for (int r = 0; r < P; r++) {
    const std::vector<int64_t> &cols = owner_cols[(size_t)r];
    // cumulative boundaries: slice c ends with the first column at which the running count reaches (c + 1) / nsl of the
    // share, so no slice exceeds its even part by more than one column
    size_t a = 0;
    int64_t run = 0;
    for (int c = 0; c < nsl; c++) {
      const int64_t goal = (share[(size_t)r] * (c + 1) + nsl - 1) / nsl;
      size_t b = a;
      int64_t n = 0;
      while (b < cols.size() && (run + n < goal || c == nsl - 1)) n += col_tiles[(size_t)cols[b++]];
      slices[(size_t)r].push_back({(int64_t)a, (int64_t)b});
      seg = std::max(seg, n);
      run += n;
      a = b;
    }
  }
  int bufs = 2;
  if (2 * P * seg > budget + 2 * nt) bufs = 1;  // two buffers do not fit (slices are whole tile columns): one, the transfer in line
  w->assembly_rs = true;
  w->stage_bufs = bufs;
  w->stage_tiles = (int64_t)bufs * P * seg;
  w->chunks.clear();
  std::vector<std::vector<int64_t>> cco;
  std::vector<int> col_chunk((size_t)nt, -1);
  for (int c = 0; c < nsl; c++) {
    SchurChunk ch;
    ch.owner = -1;
    ch.seg = seg;
    ch.ntiles = (int64_t)P * seg;
    std::vector<int64_t> table((size_t)nt, BA_NO_TILE);
    bool any = false;
    for (int r = 0; r < P; r++) {
      const std::vector<int64_t> &cols = owner_cols[(size_t)r];
      const auto sl = slices[(size_t)r][(size_t)c];
      if (sl.first >= sl.second) continue;
      any = true;
      const int64_t t0 = local_off[(size_t)cols[(size_t)sl.first]];
      int64_t n = 0;
      for (int64_t a = sl.first; a < sl.second; a++) {
        const int64_t j = cols[(size_t)a];
        table[(size_t)j] = (int64_t)r * seg + (local_off[(size_t)j] - t0);
        col_chunk[(size_t)j] = (int)w->chunks.size();
        n += col_tiles[(size_t)j];
      }
      if (r == me) {
        ch.my_t0 = t0;
        ch.my_n = n;
      }
    }
    if (!any) continue;
    w->chunks.push_back(std::move(ch));
    cco.push_back(table);
  }
  for (int q = 0; q < 2; q++) {
    if (!w->ev_stage_ready[q]) BA_CHECK(w->ev_stage_ready[q].create(hipEventDisableTiming));
    if (!w->ev_stage_free[q]) BA_CHECK(w->ev_stage_free[q].create(hipEventDisableTiming));
  }
  return upload_chunk_tables(w, cco, col_chunk, w->use_pattern);
}

static int build_chunks(ba_problem *p, LMWork *w) {
  const DenseLDL &l = w->ldl;
  const int64_t nt = l.nt;
  const int P = l.world;
  // block-sparse S: a tile column holds the pattern's tiles only (h_col_cnt) and the chunk tables are compressed like the
  // workspace's own (head nt, column offsets, the shared nt x nt row positions)
  const bool sparse = w->use_pattern;
  std::vector<int64_t> col_tiles((size_t)nt);
  std::vector<std::vector<int64_t>> owner_cols((size_t)P);
  for (int64_t j = 0; j < nt; j++) {
    col_tiles[(size_t)j] = sparse ? l.h_col_cnt[(size_t)j] : nt - j;
    owner_cols[(size_t)((j / 2) % P)].push_back(j);
  }
  const char *e = getenv("BA_ASSEMBLY");  // reduce: every chunk onto ONE owner (round 3's form); default: reduce-scatter
  if (!(e && strcmp(e, "reduce") == 0)) return build_chunks_rs(w, owner_cols, col_tiles);
  std::vector<int> col_chunk((size_t)nt, -1);
  std::vector<std::vector<int64_t>> cco;
  w->chunks.clear();
  w->stage_tiles = 0;
  for (int r = 0; r < P; r++) {
    const int64_t t_begin = l.own_range[(size_t)r], t_end = l.own_range[(size_t)r + 1], share = t_end - t_begin;
    const int64_t target = std::max<int64_t>(1, (share + 1) / 2);
    SchurChunk c;
    c.owner = r;
    c.t0 = 0;
    std::vector<int64_t> table((size_t)nt, BA_NO_TILE);
    int64_t local = 0;  // tile offset inside rank r's own layout
    auto flush = [&]() {
      if (c.ntiles == 0) return;
      if (r != l.rank) w->stage_tiles = std::max(w->stage_tiles, c.ntiles);
      w->chunks.push_back(std::move(c));
      cco.push_back(table);
      c = SchurChunk();
      c.owner = r;
      c.t0 = local;
      std::fill(table.begin(), table.end(), BA_NO_TILE);
    };
    for (int64_t j : owner_cols[(size_t)r]) {
      const int64_t colt = col_tiles[(size_t)j];
      if (c.ntiles > 0 && c.ntiles + colt > target) flush();
      table[(size_t)j] = local - c.t0;  // offset of tile (j, j) inside the chunk's destination buffer
      col_chunk[(size_t)j] = (int)w->chunks.size();
      c.ntiles += colt;
      local += colt;
    }
    flush();
  }
  return upload_chunk_tables(w, cco, col_chunk, sparse);
}

// the keys of every chunk, its offset table on the device, the staging buffer
static int upload_chunk_tables(LMWork *w, std::vector<std::vector<int64_t>> &cco, const std::vector<int> &col_chunk, bool sparse) {
  const DenseLDL &l = w->ldl;
  const int64_t nt = l.nt;
  const SchurTasks &T = w->tasks;
  // keys per chunk (a block touches tile columns 9 cb / NB and (9 cb + 8) / NB)
  const size_t nc = w->chunks.size();
  std::vector<std::vector<int>> keys(nc), skeys(nc);
  std::vector<int> split_index(T.h_key_cb.size(), -1);
  for (size_t q = 0; q < T.h_skey.size(); q++) split_index[(size_t)T.h_skey[q]] = (int)q;
  for (size_t k = 0; k < T.h_key_cb.size(); k++) {
    const int64_t c0 = 9 * (int64_t)T.h_key_cb[k];
    const int ch0 = col_chunk[(size_t)(c0 / NB)], ch1 = col_chunk[(size_t)((c0 + 8) / NB)];
    for (int ch : {ch0, ch1 == ch0 ? -1 : ch1}) {
      if (ch < 0) continue;
      if (split_index[k] >= 0) skeys[(size_t)ch].push_back(split_index[k]);
      else keys[(size_t)ch].push_back((int)k);
    }
  }
  for (size_t c = 0; c < nc; c++) {
    SchurChunk &ch = w->chunks[c];
    {  // (tix reads the head of a table one entry before its pointer: 0 = dense columns, nt = compressed ones)
      std::vector<int64_t> with_head(cco[c].size() + 1 + (sparse ? (size_t)(nt * nt) : 0), 0);
      std::copy(cco[c].begin(), cco[c].end(), with_head.begin() + 1);
      if (sparse) {
        with_head[0] = nt;
        std::copy(l.h_col_tab.begin() + 1 + nt, l.h_col_tab.end(), with_head.begin() + 1 + nt);
      }
      BA_CHECK(upload(ch.cco_alloc, with_head));
      ch.cco = ch.cco_alloc + 1;
    }
    BA_CHECK(upload(ch.keys, keys[c]));
    BA_CHECK(upload(ch.skeys, skeys[c]));
    ch.nkeys = (int64_t)keys[c].size();
    ch.nskeys = (int64_t)skeys[c].size();
  }
  BA_CHECK(w->stage.alloc(std::max<int64_t>(1, w->stage_tiles) * NB * NB));
  return BA_OK;
}

// OR of a flag array over the ranks (set-up only): as doubles through the all-reduce the transport has
static int allreduce_flags(ba_problem *p, std::vector<unsigned char> *flags) {
  if (!p->comm.active() || flags->empty()) return BA_OK;
  std::vector<double> h(flags->begin(), flags->end());
  DevBuf<double> d;
  BA_CHECK(d.alloc((int64_t)h.size()));
  BA_HIP_CHECK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  BA_CHECK(comm_allreduce(p, d, (int64_t)h.size(), p->stream));
  BA_HIP_CHECK(hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  BA_HIP_CHECK(hipStreamSynchronize(p->stream));
  for (size_t i = 0; i < h.size(); i++) (*flags)[i] = h[i] != 0.0;
  return BA_OK;
}

// OR of the camera graph over the ranks: a rank's observations only show the camera pairs ITS points connect, the ordering
// must be that of the whole problem and the same on every rank.  The bit rows travel as counts, eight 6-bit fields per
// double (a field holds at most `world` <= 63), in slices of at most 128 MB.
static int allreduce_cam_graph(ba_problem *p, CamGraph *g) {
  if (!p->comm.active() || g->bits.empty()) return BA_OK;
  const size_t nwords = g->bits.size(), ndbl = nwords * 8;
  const size_t slice = std::min<size_t>(ndbl, (size_t)16 << 20);
  std::vector<double> h(slice);
  DevBuf<double> d;
  BA_CHECK(d.alloc((int64_t)slice));
  for (size_t off = 0; off < ndbl; off += slice) {
    const size_t cnt = std::min(slice, ndbl - off);
    for (size_t i = 0; i < cnt; i++) {  // double off + i: byte ((off + i) & 7) of word (off + i) / 8
      const uint64_t byte = (g->bits[(off + i) >> 3] >> (8 * ((off + i) & 7))) & 0xff;
      uint64_t packed = 0;
      for (int b = 0; b < 8; b++) packed |= ((byte >> b) & 1) << (6 * b);
      h[i] = (double)packed;
    }
    BA_HIP_CHECK(hipMemcpyAsync(d, h.data(), cnt * sizeof(double), hipMemcpyHostToDevice, p->stream));
    BA_CHECK(comm_allreduce(p, d, (int64_t)cnt, p->stream));
    BA_HIP_CHECK(hipMemcpyAsync(h.data(), d, cnt * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    BA_HIP_CHECK(hipStreamSynchronize(p->stream));
    for (size_t i = 0; i < cnt; i++) {
      const uint64_t packed = (uint64_t)h[i];
      uint64_t byte = 0;
      for (int b = 0; b < 8; b++) byte |= (uint64_t)(((packed >> (6 * b)) & 63) != 0) << b;
      uint64_t &word = g->bits[(off + i) >> 3];
      const int sh = 8 * (int)((off + i) & 7);
      word = (word & ~((uint64_t)0xff << sh)) | (byte << sh);
    }
  }
  return BA_OK;
}

// Fill-reducing ordering of the cameras inside the reduced camera system -- what `perm` asks of the reference's sparse
// LDL' (amd(A) / Metis.permutation, src/lm.jl:84-88, consumed by ldl_analyse, src/ldl_aux.jl:246-283).  The tile pattern of S
// depends on how the cameras are numbered; a BAL file promises nothing about that.  Cameras keep their numbers everywhere
// else (x, J, Hcc, gc): only S, its right-hand side and its solution live in the new order (SchurTasks::cam_of / pos).
// pos_out: block row of every camera, empty when the caller's numbering stays.
static int order_cameras(ba_problem *p, LMWork *w, std::vector<int> *pos_out) {
  pos_out->clear();
  w->h_cam_perm.clear();
  w->order_name = "natural";
  w->order_split = 0;
  int method = w->order_method;
  if (const char *e = getenv("BA_CAM_ORDER")) {  // amd | metis | natural: overrides the handle's setting (experiments)
    method = e[0] == 'n' ? BA_ORDER_NATURAL : (e[0] == 'm' ? BA_ORDER_METIS : BA_ORDER_AMD);
  }
  const int64_t n = p->ncams;
  // (fewer cameras than two tiles hold: dense anyway; several ranks: with per-rank ownership of S only, and at most 63 ranks
  // -- the graph's bits are summed as 6-bit counts)
  if (method == BA_ORDER_NATURAL || n < 2 * (NB / 9)) return BA_OK;
  if (p->comm.active() && (!w->ldl.own_only || p->comm.world > 63)) return BA_OK;
  CamGraph g;
  cam_graph_build(n, p->npnts, p->h_pt_ptr.data(), p->h_pt_obs.data(), p->h_cam0.data(), &g);
  BA_CHECK(allreduce_cam_graph(p, &g));
  // more than half of all camera pairs share points: S is dense at tile granularity whatever the order
  if ((double)g.edges() > 0.25 * (double)n * (double)(n - 1)) return BA_OK;
  std::vector<int> perm;
  const char *name = "natural";
  int split = 0;
  cam_order(g, method, NB, &perm, &name, &split);
  bool identity = true;
  for (int64_t k = 0; k < n && identity; k++) identity = perm[(size_t)k] == (int)k;
  if (identity) return BA_OK;
  w->order_name = name;
  w->order_split = split;
  pos_out->resize((size_t)n);
  for (int64_t k = 0; k < n; k++) (*pos_out)[(size_t)perm[(size_t)k]] = (int)k;
  BA_CHECK(upload(w->tasks.cam_of, perm));
  BA_CHECK(upload(w->tasks.pos, *pos_out));
  w->h_cam_perm.swap(perm);
  return BA_OK;
}

// what only the direct solves need: the tiles of S, the Schur task list, the per-observation Y blocks
static int ensure_dense(ba_problem *p, LMWork *w) {
  if (w->ldl.own_tiles) return BA_OK;  // (made behind S: a call that failed before it is redone whole)
  BA_CHECK(w->Yobs.alloc(6 * p->nobs));
  std::vector<int> pos;
  BA_CHECK(order_cameras(p, w, &pos));
  BA_CHECK(build_tasks(p, &w->tasks, pos));
  // Block-sparse reduced camera system (one GPU): symbolic factorisation of the tile occupancy; the list schedule is used
  // when the pattern's trailing updates are at most 60 % of the dense factorisation's (BA_SPARSE_S=1 / 0 forces it on /
  // off).  Every camera pair sharing points (the default synthetic generator, small problems) gives flop_fill = 1: dense.
  // several ranks: a rank's keys only show the tiles ITS observations touch; the pattern is that of the sum
  if (dist_factor_on(p)) BA_CHECK(allreduce_flags(p, &w->tasks.tile_occ));
  tile_pattern_build(w->ldl.nt, w->tasks.tile_occ, &w->pattern, w->order_split);
  w->tasks.tile_occ.clear();
  w->tasks.tile_occ.shrink_to_fit();
  const char *e = getenv("BA_SPARSE_S");
  const bool want = e ? e[0] != '0' : (w->pattern.flop_fill <= 0.6 && w->ldl.nt >= 8);
  w->use_pattern = want && (!p->comm.active() || w->ldl.own_only);  // (several ranks: with per-rank ownership of S only)
  if (w->use_pattern) BA_CHECK(dense_ldl_use_pattern(&w->ldl, &w->pattern));  // (compressed layout: before S is allocated)
  BA_CHECK(dense_ldl_alloc_S(&w->ldl));
  // (the layout is final: the tile list of the column scaling and the border's masking; the Float32 twin is never scaled)
  BA_CHECK(dense_ldl_list_tiles(&w->ldl));
  if (w->ldl.own_only) return build_chunks(p, w);
  w->whole.ntiles = w->ldl.s_tiles;
  w->whole.cco = w->ldl.col_off;
  w->whole.nkeys = w->tasks.nkeys;
  w->whole.nskeys = w->tasks.nsplit;
  return BA_OK;
}

// shared intrinsics, direct path: the grouping's tables in the order of S and the border buffers
static int ensure_shared_direct(ba_problem *p, LMWork *w) {
  if (!p->grp_on() || w->grp_made_for == p->grp_version) return BA_OK;
  std::vector<int> pos;  // block row of a camera
  if (!w->h_cam_perm.empty()) {
    pos.resize(w->h_cam_perm.size());
    for (size_t k = 0; k < pos.size(); k++) pos[(size_t)w->h_cam_perm[k]] = (int)k;
  }
  std::vector<int> row(p->h_grp_mem.size()), col((size_t)w->npad, -1);
  for (int g = 0; g < p->grp_n; g++)
    for (int m = p->h_grp_ptr[(size_t)g]; m < p->h_grp_ptr[(size_t)g + 1]; m++) {
      const int c = p->h_grp_mem[(size_t)m];
      row[(size_t)m] = 9 * (pos.empty() ? c : pos[(size_t)c]) + 6;
      for (int q = 0; q < 3; q++) col[(size_t)(row[(size_t)m] + q)] = 3 * g + q;
    }
  BA_CHECK(upload(w->grp_row, row));
  BA_CHECK(upload(w->grp_col, col));
  if (!w->bord_small) {
    BA_CHECK(w->bord_B.alloc(24 * w->npad));
    BA_CHECK(w->bord_Y.alloc(24 * w->npad));
    BA_CHECK(w->bord_w.alloc(24 * w->npad));
    BA_CHECK(w->bord_small.alloc(SHARED_SMALL_DOUBLES));
  }
  w->grp_made_for = p->grp_version;
  return BA_OK;
}

void lm_free(ba_problem *p) {
  delete p->lm;
  p->lm = nullptr;
}

// the partial sums of S held by every rank -> the complete tile columns on their owners (distributed factorisation), or
// the complete S everywhere (replicated); the right-hand side is needed by every rank either way
// s32: the factorisation will run in Float32 and nothing needs the Float64 sum (no column scaling): every rank rounds its
// partial sums to Float32 first and the owners receive Float32 sums -- half the bytes of the largest transfer of the
// iteration (Final-13682: 30 GB instead of 60); the sum of `world` rounded partials differs from the rounded sum by a few
// Float32 ulps, the level of the factorisation itself.
static int reduce_camera_system(ba_problem *p, LMWork *w, hipStream_t st, bool s32) {
  if (!p->comm.active()) return BA_OK;
  if (!dist_factor_on(p)) {  // replicated: the whole S and the right-hand side everywhere
    BA_CHECK(comm_allreduce(p, w->ldl.S, w->ldl.s_tiles * NB * NB, st));
    return comm_allreduce(p, w->rhs, w->npad, st);
  }
  if (s32) BA_CHECK(launch_convert(w->ldl.S, w->ldl32.S, w->ldl.s_tiles * NB * NB, st));
  BA_CHECK(comm_group_begin(p));
  int rc = BA_OK;
  for (int r = 0; r < w->ldl.world && rc == BA_OK; r++) {
    const int64_t b = w->ldl.own_range[(size_t)r], e = w->ldl.own_range[(size_t)r + 1];
    rc = s32 ? comm_reduce_f32(p, w->ldl32.S + b * NB * NB, (e - b) * NB * NB, r, st)
             : comm_reduce(p, w->ldl.S + b * NB * NB, (e - b) * NB * NB, r, st);
  }
  BA_CHECK(comm_group_end(p));
  BA_CHECK(rc);
  return comm_allreduce(p, w->rhs, w->npad, st);
}

// r, J and the normal-equation blocks at w->x; fills sharded/replicated scalars RSQ?, GP, GC, X_P, X_C (and RTSQ)
// recorded: the last reduction kernel also writes the controller's scalars to the pinned host buffers
// Under a robust loss r and J are reweighted in place (r~, J~) before anything reads them; r must hold the plain residual at
// w->x on entry (residual_too, or the trial residual of an accepted step).  With per-observation information
// (ba_lm_set_obs_info) the same pass (k_obs_scale) whitens them: r^ and J^, the loss's reweighting on top; the trial residual
// of an accepted step is whitened already (trial_point)
static int refresh_linearisation(ba_problem *p, LMWork *w, bool residual_too, bool recorded, hipStream_t st) {
  if (w->mode.xf32) {  // w->x holds Float32 values: evaluate with the Float32 kernels, widen (exact)
    BA_CHECK(launch_convert(w->x, w->xf, w->nvar, st));
    if (residual_too) {
      BA_CHECK(launch_residual_f32(p, w->xf, w->rf, st));
      BA_CHECK(launch_convert(w->rf, w->r, w->nequ, st));
    }
    BA_CHECK(launch_jac_coord_f32(p, w->xf, w->Jf, st));
    BA_CHECK(launch_convert(w->Jf, w->J, 24 * p->nobs, st));
  } else {
    if (residual_too) BA_CHECK(launch_residual_f64(p, w->x, w->r, st));
    BA_CHECK(launch_jac_coord_f64(p, w->x, w->J, st));
  }
  if (p->fix_on()) BA_CHECK(launch_fix_mask(p, w->J, st));  // fixed parameters (ba_lm_set_fixed): their columns of J to 0
  const bool robust = p->loss != BA_LOSS_LINEAR;  // (never with xf32: refused by ba_lm_solve)
  // (its partial sums are read under a loss only: the linear loss sums w->r below)
  BA_CHECK(launch_obs_scale(p, w->r, w->J, nullptr, robust ? (double *)w->rob_partial : nullptr, residual_too, true, st));
  BA_CHECK(launch_point_blocks(p, w->J, w->r, w->Hpp, w->gp, st));
  BA_CHECK(launch_cam_blocks(p, w->J, w->r, w->Hcc, w->gc, st));
  // priors (ba_lm_set_priors): their terms into the diagonal blocks and the gradient, before anything reads either
  BA_CHECK(launch_prior_lin(p, w->x, w->Hpp, w->gp, w->Hcc, w->gc, st));
  // shared intrinsics: the gradient over z -- a group's sum at its first member, exact zeros at the others (nothing but the
  // gradient output and its norm reads gc)
  if (p->grp_on()) BA_CHECK(launch_grp_reduce(p, p->grp_ptr, p->grp_row, w->gc, st));
  // gc, the diagonal of the camera block (the column scalings need the global one) and the linearisation scalars are
  // adjacent in the reduce buffer (lm_ensure): one all-reduce
  BA_CHECK(launch_hcc_diag(p, w->Hcc, w->hdiag, st));
  // |r|^2, |gp|^2, |x_points|^2 and -- of the all-reduced gc -- |gc|^2, |x_cameras|^2: one launch pair on one rank, two with a
  // communicator (the camera sums wait for the all-reduce); the same bits per vector either way
  SumsqJobs jobs;
  if (robust) {  // 2 f and |r~|^2 from k_obs_scale's partials
    const int nb = obs_blocks(p->nobs);
    jobs.add_sum(w->rob_partial, nb, w->scal, SH_RSQ);
    jobs.add_sum(w->rob_partial + RED_BLOCKS, nb, w->scal, SH_RTSQ);
  } else {
    jobs.add(w->r, w->nequ, w->scal, SH_RSQ);
  }
  if (p->pri_on()) {  // + 2 f_prior where the controller reads 2 f (and |r~|^2, the zero-step model value)
    jobs.add_sum(p->pri_cost(), p->pri_total(), w->scal, SH_RSQ, true);
    if (robust) jobs.add_sum(p->pri_cost(), p->pri_total(), w->scal, SH_RTSQ, true);
  }
  jobs.add(w->gp, 3 * p->npnts, w->scal, SH_GP);
  jobs.add(w->x, 3 * p->npnts, w->scal, SH_X_P);
  if (p->comm.active()) {
    BA_CHECK(launch_sumsq_multi(p, &jobs, w->partial_multi, st));
    BA_CHECK(comm_allreduce(p, w->gc, 2 * w->npad + SH_LIN_COUNT + (robust ? 1 : 0), st));  // (+ SH_RTSQ)
    jobs = SumsqJobs();
  }
  if (w->mode.f16) BA_CHECK(launch_col_sq(p, w->Hpp, w->hdiag, w->jn2, st));  // |J_j|^2 before the blocks are overwritten by scaled ones
  jobs.add(w->gc, w->n, w->scal_rep, RP_GC);
  jobs.add(w->x + 3 * p->npnts, w->n, w->scal_rep, RP_X_C);
  if (recorded) jobs.publish(w->scal, SH_COUNT, w->h_sh, w->scal_rep, RP_COUNT, w->h_rp, nullptr, nullptr);
  BA_CHECK(launch_sumsq_multi(p, &jobs, w->partial_multi, st));
  return BA_OK;
}

static int fetch_scalars(ba_problem *p, LMWork *w, hipStream_t st) {
  BA_CHECK(launch_publish(w->scal, SH_COUNT, w->h_sh, w->scal_rep, RP_COUNT, w->h_rp, nullptr, nullptr, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

// ---- facto = PCG ------------------------------------------------------------------------------------------------------
// The reference has no iterative branch (its solves are sparse direct, src/lm.jl:61-112); SURVEY 8(f) lists PCG on the
// reduced camera system as the way to Final-scale problems, where the dense S (60 GB for Final-13682) and its n^3/3 flops
// stop paying.  Here S = Hcc + lambda I - W U^-1 W' is applied, never formed: two sweeps over J per product (the
// back-substitution pass by point, the right-hand-side pass by camera), preconditioned by its 9 x 9 diagonal blocks.  On
// several ranks the product is summed by ONE all-reduce of 9 ncams doubles per CG iteration; everything else is replicated.
static int ensure_pcg(ba_problem *p, LMWork *w) {
  if (w->h_cg) return BA_OK;  // (the last allocation: a failed call is redone whole)
  auto dm = [](DevBuf<double> &q, int64_t cnt) -> int {
    BA_CHECK(q.alloc(cnt));
    BA_HIP_CHECK(hipMemset(q, 0, (size_t)(cnt > 0 ? cnt : 1) * sizeof(double)));
    return BA_OK;
  };
  for (DevBuf<double> *q : {&w->cgx, &w->cgr, &w->cgz, &w->cgp, &w->cgq, &w->cgt}) BA_CHECK(dm(*q, w->npad));
  BA_CHECK(dm(w->cgh, 3 * p->npnts));
  BA_CHECK(dm(w->zero3, 3 * p->npnts));
  BA_CHECK(dm(w->blk45, 45 * p->ncams));
  BA_CHECK(dm(w->cg_scal, 8));
  BA_HIP_CHECK(hipDeviceSynchronize());  // (the null-stream memsets above are not ordered against the handle's stream)
  BA_CHECK(w->h_cg.alloc(8));
  return BA_OK;
}

// shared intrinsics: q = (E'(S_full - lambda I)E + lambda I) v for v over z: expand, the product without damping, reduce, damp
static int pcg_matvec_shared(ba_problem *p, LMWork *w, double lambda, const double *v, double *q, hipStream_t st) {
  BA_HIP_CHECK(hipMemcpyAsync(w->cge, v, (size_t)w->n * sizeof(double), hipMemcpyDeviceToDevice, st));
  BA_CHECK(launch_grp_expand(p, p->grp_ptr, p->grp_row, w->cge, st));
  if (p->point_sorted) BA_CHECK(launch_wtv(p, w->J, w->Uinv, w->cge, w->cgh, st));
  else BA_CHECK(launch_backsub(p, w->J, w->Uinv, w->zero3, w->cge, w->cgh, st));
  BA_CHECK(launch_wuw(p, w->J, w->cgh, w->Hcc, w->cge, 0.0, q, st, w->cam_pnt));
  BA_CHECK(launch_grp_reduce(p, p->grp_ptr, p->grp_row, q, st));
  return launch_axpy_s(p, w->n, lambda, v, q, st);
}

// q = S v: the point sweep, then the camera sweep (which adds Hcc v and, on one rank, the damping); on several ranks the
// partial products are summed by one all-reduce and every rank adds the damping to the full sum
static int pcg_matvec(ba_problem *p, LMWork *w, double lambda, const double *v, double *q, hipStream_t st) {
  const bool shared = p->comm.active();
  if (p->point_sorted) BA_CHECK(launch_wtv(p, w->J, w->Uinv, v, w->cgh, st));  // h = -U^-1 W' v
  else BA_CHECK(launch_backsub(p, w->J, w->Uinv, w->zero3, v, w->cgh, st));  // (observations not grouped by point)
  BA_CHECK(launch_wuw(p, w->J, w->cgh, w->Hcc, v, shared ? 0.0 : lambda, q, st, w->cam_pnt));
  if (!shared) return BA_OK;
  BA_CHECK(comm_allreduce(p, q, w->n, st));
  return launch_axpy_s(p, w->n, lambda, v, q, st);
}

static int pcg_fetch(LMWork *w, hipStream_t st) {
  BA_HIP_CHECK(hipMemcpyAsync(w->h_cg, w->cg_scal, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

// S x = rhs (w->rhs in, solution out) to |r| <= pcg_tol |rhs| or pcg_maxit iterations.  alpha and beta are formed on the
// device (k_cg_alpha, k_cg_beta_dir); the host reads the scalars once per iteration, for the stopping test.
static int pcg_solve(ba_problem *p, LMWork *w, double lambda, hipStream_t st) {
  BA_CHECK(ensure_pcg(p, w));
  const int64_t n = w->n;
  const int maxit = w->mode.pcg_maxit > 0 ? w->mode.pcg_maxit : 1000;
  BA_HIP_CHECK(hipMemsetAsync(w->ldl.flag, 0, sizeof(int), st));
  BA_CHECK(launch_schur_diag(p, w->J, w->Uinv, w->Hcc, w->blk45, st));
  BA_CHECK(comm_allreduce(p, w->blk45, 45 * p->ncams, st));
  const bool shared = p->grp_on();  // shared intrinsics: the system over z, its vectors in the x layout (zeros at non-first members)
  if (shared) {
    if (!w->cge) BA_CHECK(w->cge.alloc(w->npad));
    BA_CHECK(launch_grp_blk45(p, w->blk45, st));
  }
  BA_CHECK(launch_pcg_factor(p, lambda, w->blk45, w->ldl.flag, st));  // a block that is not positive definite -> SQDException
  BA_HIP_CHECK(hipMemsetAsync(w->cgx, 0, (size_t)n * sizeof(double), st));
  BA_HIP_CHECK(hipMemcpyAsync(w->cgr, w->rhs, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  BA_CHECK(launch_cg_step(p, w->cg_scal, w->blk45, w->cgp, w->cgq, w->cgx, w->cgr, w->cgz, w->cgt, 1, st));  // z, r.r, r.z
  BA_CHECK(launch_cg_beta_dir(p, n, w->cgt, w->cg_scal, w->cgz, w->cgp, 1, st));                              // p = z
  BA_CHECK(pcg_fetch(w, st));
  const double b2 = w->h_cg[1];
  int it = 0;
  if (b2 > 0 && w->h_cg[2] == w->h_cg[2]) {
    for (it = 1; it <= maxit; it++) {
      BA_CHECK(shared ? pcg_matvec_shared(p, w, lambda, w->cgp, w->cgq, st) : pcg_matvec(p, w, lambda, w->cgp, w->cgq, st));
      BA_CHECK(launch_cg_alpha(p, n, w->cgp, w->cgq, w->cg_scal, st));
      BA_CHECK(launch_cg_step(p, w->cg_scal, w->blk45, w->cgp, w->cgq, w->cgx, w->cgr, w->cgz, w->cgt, 0, st));
      BA_CHECK(launch_cg_beta_dir(p, n, w->cgt, w->cg_scal, w->cgz, w->cgp, 0, st));
      BA_CHECK(pcg_fetch(w, st));
      const double pq = w->h_cg[0], rr = w->h_cg[1];
      // p.q <= 0: S not positive definite along p (or NaN) -- alpha was 0, nothing moved; keep what there is, the LM test
      // judges the step
      if (!(pq > 0) || !(rr == rr) || rr <= w->mode.pcg_tol * w->mode.pcg_tol * b2) break;
    }
  }
  w->n_cg += it < maxit ? it : maxit;
  BA_HIP_CHECK(hipMemcpyAsync(w->rhs, w->cgx, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  return BA_OK;
}

// ---- the linear step, part by part (linear_step below runs them in this order) ---------------------------------------------
constexpr double MU16 = 0.1 * 6.55e4;  // lma_aux.jl:44-48
// facto_type = Float16: columns scaled by their norms, entries and right-hand side rounded to Float16 (k_f16_cols); the
// normal-equation blocks are rebuilt from the rounded copies (J_lin / r_lin from here on), the damping is per column (w->damp)
static int f16_prepare(ba_problem *p, LMWork *w, double lambda, hipStream_t st) {
  BA_CHECK(launch_f16_scale(p, lambda, MU16, w->jn2, w->J, w->r, w->dcol, w->damp, w->Jq, w->rq, st));
  BA_CHECK(launch_point_blocks(p, w->Jq, w->rq, w->Hpp, w->gp, st));
  return launch_cam_blocks(p, w->Jq, w->rq, w->Hcc, w->gc, st);
}

// U^-1 and u of every point at the damping; recorded: the damping is read from h_lambda and left in d_lambda on the way
static int eliminate_points(ba_problem *p, LMWork *w, double lambda, const double *damp, bool recorded, hipStream_t st) {
  // (single-rank direct path: the right-hand side buffer is cleared by this kernel instead of a memset node of its own)
  const bool rhs_here = !w->mode.pcg && !w->ldl.own_only;
  // recorded sequences read the damping from pinned host memory (h_lambda).  In k_schur_prep every wave would fetch that
  // scalar over PCIe -- unnoticeable for the few thousand waves of a small problem, where the saved copy node pays, but 15 k
  // waves on the Venice shape and 70 k on Final-13682's: there one thread copies it to device memory first
  double *const hl = w->h_lambda, *const dl = w->d_lambda;
  const bool from_host = recorded && p->npnts <= 200000;
  if (recorded && !from_host) BA_CHECK(launch_publish(hl, 1, dl, nullptr, 0, nullptr, nullptr, nullptr, st));
  return launch_schur_prep(p, lambda, w->Hpp, w->gp, w->Uinv, w->u, st, from_host ? hl : (recorded ? dl : nullptr), damp,
                           from_host ? dl : nullptr, rhs_here ? w->rhs : nullptr, rhs_here ? w->npad : 0);
}

// facto = PCG: the reduced camera system is applied, not formed (pcg_solve); no column scaling: block Jacobi has its own
static int pcg_step(ba_problem *p, LMWork *w, double lambda, hipStream_t st) {
  BA_HIP_CHECK(hipMemsetAsync(w->rhs, 0, (size_t)w->npad * sizeof(double), st));
  BA_CHECK(launch_schur_rhs(p, w->J_lin(), w->r_lin(), w->u, w->rhs, st, w->cam_pnt));
  BA_CHECK(launch_prior_rhs(p, w->rhs, nullptr, st));  // - H'Lambda d of the camera and centre priors
  BA_CHECK(comm_allreduce(p, w->rhs, w->npad, st));
  if (p->grp_on()) BA_CHECK(launch_grp_reduce(p, p->grp_ptr, p->grp_row, w->rhs, st));  // E' rhs
  BA_CHECK(pcg_solve(p, w, lambda, st));
  double *dcp = w->delta + 3 * p->npnts;
  BA_HIP_CHECK(hipMemcpyAsync(dcp, w->rhs, (size_t)w->n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (p->grp_on()) BA_CHECK(launch_grp_expand(p, p->grp_ptr, p->grp_row, dcp, st));  // dx = E dz
  return launch_backsub(p, w->J_lin(), w->Uinv, w->u, dcp, w->delta, st, w->r_lin(), w->cr0(), w->partial, w->scal, SH_MODEL,
                        &w->model_done);
}

// the 9 x 9 blocks of one chunk of S into dest, cleared first (behind launch_schur_pre; the unit diagonal of the padding rows
// by rank 0)
static int assemble_chunk(ba_problem *p, LMWork *w, const SchurChunk &c, double *dest, double lam_diag, const double *d_lambda,
                          const double *damp, hipStream_t st) {
  ProfScope ps(p, PC_SCHUR_S, st);
  BA_HIP_CHECK(hipMemsetAsync(dest, 0, (size_t)c.ntiles * NB * NB * sizeof(double), st));
  return launch_schur_chunk(p, &w->tasks, &c, w->J_lin(), w->Yobs, w->Hcc, lam_diag, dest, w->n, p->rank == 0 ? w->npad : w->n, st,
                            d_lambda, damp, false);
}

// S of a rank that holds all of it: every 9 x 9 block straight into the tiles, the whole matrix as one chunk (this rank's
// partial sums: reduce_camera_system).  One profiling scope over all of it.  The launches keep the order this assembly has
// always had -- zero-fill of S, k_obs_y, short keys, partial sums of the split keys, their sums.  The order means nothing to
// the result; the zero-fill behind k_obs_y and the partial sums ahead of the short keys were both tried on the Venice shape
// and neither measured faster (the class time 0.2 % and 2 % above this order's, at a spread of 0.1 % and 1 %)
static int assemble_local(ba_problem *p, LMWork *w, double lam_diag, const double *d_lambda, const double *damp, hipStream_t st) {
  ProfScope ps(p, PC_SCHUR_S, st);
  BA_HIP_CHECK(hipMemsetAsync(w->ldl.S, 0, (size_t)w->whole.ntiles * NB * NB * sizeof(double), st));
  BA_CHECK(launch_schur_pre(p, &w->tasks, w->J_lin(), w->Uinv, w->Yobs, st, false));
  return launch_schur_chunk(p, &w->tasks, &w->whole, w->J_lin(), w->Yobs, w->Hcc, lam_diag, w->ldl.S, w->n,
                            p->rank == 0 ? w->npad : w->n, st, d_lambda, damp, true);
}

// per-rank ownership of S: chunk by chunk -- this rank's share of the chunk's sums goes straight into its own tiles
// when it owns the chunk, else into the staging buffer -- and every chunk is reduced onto its owner at once
static int assemble_chunks_reduce(ba_problem *p, LMWork *w, double lam_diag, const double *d_lambda, const double *damp, bool reduce32,
                                  hipStream_t st) {
  for (const SchurChunk &c : w->chunks) {
    const bool mine = c.owner == w->ldl.rank;
    double *dest = mine ? w->ldl.S + c.t0 * NB * NB : w->stage;
    BA_CHECK(assemble_chunk(p, w, c, dest, lam_diag, d_lambda, damp, st));
    if (reduce32) {  // Float32 factorisation without column scaling: the partial sums travel as Float32
      float *d32 = mine ? w->ldl32.S + c.t0 * NB * NB : w->stage32;
      BA_CHECK(launch_convert(dest, d32, c.ntiles * NB * NB, st));
      BA_CHECK(comm_reduce_f32(p, d32, c.ntiles * NB * NB, c.owner, st));
    } else {
      BA_CHECK(comm_reduce(p, dest, c.ntiles * NB * NB, c.owner, st));
    }
  }
  return BA_OK;
}

// reduce-scatter form (build_chunks_rs): every chunk is one slice of EVERY owner's columns, assembled into a staging
// buffer of `world` segments and reduce-scattered in place; the owner copies its segment into its tiles.  With two
// buffers the transfer of chunk c (transfer stream) runs beside the assembly of chunk c+1 (main stream).
static int assemble_chunks_rs(ba_problem *p, LMWork *w, double lam_diag, const double *d_lambda, const double *damp, bool reduce32,
                              hipStream_t st) {
  const int bufs = w->stage_bufs, me = w->ldl.rank;
  const int64_t buf_elems = (w->stage_tiles / bufs) * NB * NB;
  const size_t elem = reduce32 ? sizeof(float) : sizeof(double);
  char *S_own = reduce32 ? (char *)(float *)w->ldl32.S : (char *)(double *)w->ldl.S;  // this rank's tiles, in the type that travels
  hipStream_t ts = bufs == 2 ? w->ldl.hoist : st;
  bool used[2] = {false, false};
  int ci = 0;
  for (const SchurChunk &c : w->chunks) {
    const int b = bufs == 2 ? (ci++ & 1) : 0;
    double *dst = w->stage + b * buf_elems;
    if (bufs == 2 && used[b]) BA_HIP_CHECK(hipStreamWaitEvent(st, w->ev_stage_free[b], 0));  // its last transfer is through
    BA_CHECK(assemble_chunk(p, w, c, dst, lam_diag, d_lambda, damp, st));
    const int64_t seg_elems = c.seg * NB * NB, my_elems = c.my_n * NB * NB;
    float *d32 = reduce32 ? w->stage32 + b * buf_elems : nullptr;
    if (reduce32) BA_CHECK(launch_convert(dst, d32, c.ntiles * NB * NB, st));
    char *sent = reduce32 ? (char *)d32 : (char *)dst;
    if (bufs == 2) {
      BA_HIP_CHECK(hipEventRecord(w->ev_stage_ready[b], st));
      BA_HIP_CHECK(hipStreamWaitEvent(ts, w->ev_stage_ready[b], 0));
    }
    BA_CHECK(comm_reduce_scatter(p, sent, seg_elems, reduce32, ts));
    if (my_elems > 0)
      BA_HIP_CHECK(hipMemcpyAsync(S_own + (size_t)(c.my_t0 * NB * NB) * elem, sent + (size_t)((int64_t)me * seg_elems) * elem,
                                  (size_t)my_elems * elem, hipMemcpyDeviceToDevice, ts));
    if (bufs == 2) {
      BA_HIP_CHECK(hipEventRecord(w->ev_stage_free[b], ts));
      used[b] = true;
    }
  }
  for (int b = 0; b < 2; b++)
    if (used[b]) BA_HIP_CHECK(hipStreamWaitEvent(st, w->ev_stage_free[b], 0));
  return BA_OK;
}

// :J / :A column scaling of the camera system from the GLOBAL diagonal (refresh_linearisation)
static int scale_columns(ba_problem *p, LMWork *w, double lambda, const double *d_lambda, hipStream_t st) {
  BA_CHECK(launch_cam_scale(p, w->hdiag, w->mode.normalize == 2 ? lambda : 0.0, w->colscale, st, d_lambda, w->tasks.pos));
  BA_CHECK(launch_scale_S_list(p, w->n, w->colscale, w->ldl.S, w->ldl.own_tiles, w->ldl.n_own_tiles, st));
  return launch_scale_vec(p, w->n, w->colscale, w->rhs, 1, st);
}

// factor the assembled system and solve for rhs in place; the forward substitution of rhs rides along where it can
template <typename T>
static int factor_solve(ba_problem *p, DenseLDLT<T> *l, T *rhs, bool dist, hipStream_t st) {
  if (dist) {
    BA_CHECK(dense_ldl_factor_dist<T>(p, l, st, l->own_only ? rhs : (T *)nullptr));
    return dense_ldl_solve<T>(p, l, rhs, st, l->own_only);
  }
  BA_CHECK(dense_ldl_factor<T>(p, l, st, rhs));
  return dense_ldl_solve<T>(p, l, rhs, st, true);
}

// the solution in w->rhs (block rows of S, scaled columns) -> delta: cameras in camera order, points by back-substitution
static int step_from_solution(ba_problem *p, LMWork *w, bool normalize, hipStream_t st) {
  double *dc = w->delta + 3 * p->npnts;
  if (normalize) BA_CHECK(launch_scale_vec(p, w->n, w->colscale, w->rhs, 1, st));  // dc = D^-1 dc'
  if (w->tasks.pos) BA_CHECK(launch_gather_cams(p, w->tasks.pos, w->rhs, dc, st));  // block rows of S -> camera order
  else BA_HIP_CHECK(hipMemcpyAsync(dc, w->rhs, (size_t)w->n * sizeof(double), hipMemcpyDeviceToDevice, st));
  // the model value of the step rides along with the back-substitution (not in the Float16 branch: its step is rescaled below)
  BA_CHECK(launch_backsub(p, w->J_lin(), w->Uinv, w->u, dc, w->delta, st, w->mode.f16 ? nullptr : w->r_lin(), w->cr0(), w->partial,
                          w->scal, SH_MODEL, &w->model_done));
  if (w->mode.f16) BA_CHECK(launch_scale_scalar(p, w->nvar, w->delta, 1.0 / MU16, st));  // the right-hand side was -Jh' r / mu
  return BA_OK;
}

// delta = -(J'J + lambda I)^-1 J'r at the current linearisation; also |J delta + r|^2 -> SH_MODEL, |delta|^2
// recorded: the damping is read from device memory (h_lambda -> d_lambda, eliminate_points); `lambda` is then the multiplier 1
static int linear_step(ba_problem *p, LMWork *w, double lambda, bool recorded, hipStream_t st) {
  const StepMode &m = w->mode;
  // every rank holds partial Hcc / Schur sums; the lambda I of the camera block is added by rank 0 only
  const double lam_diag = (p->rank == 0) ? lambda : 0.0;
  const double *const d_lambda = recorded ? (double *)w->d_lambda : nullptr, *const damp = m.f16 ? (double *)w->damp : nullptr;
  const bool normalize = m.normalize != 0 && !m.f16;  // lm.jl:156,232: no column scaling of J in the Float16 branch
  if (m.f16) BA_CHECK(f16_prepare(p, w, lambda, st));
  BA_CHECK(eliminate_points(p, w, lambda, damp, recorded, st));
  if (m.pcg) return pcg_step(p, w, lambda, st);
  const bool dist = dist_factor_on(p);
  const bool reduce32 = dist && m.facto_f32 && !normalize;
  if (reduce32) BA_CHECK(ensure_f32(w));
  if (w->ldl.own_only) {
    {
      ProfScope ps(p, PC_SCHUR_S, st);
      BA_CHECK(launch_schur_pre(p, &w->tasks, w->J_lin(), w->Uinv, w->Yobs, st, true));
    }
    if (w->assembly_rs) BA_CHECK(assemble_chunks_rs(p, w, lam_diag, d_lambda, damp, reduce32, st));
    else BA_CHECK(assemble_chunks_reduce(p, w, lam_diag, d_lambda, damp, reduce32, st));
    BA_HIP_CHECK(hipMemsetAsync(w->rhs, 0, (size_t)w->npad * sizeof(double), st));
  } else {
    BA_CHECK(assemble_local(p, w, lam_diag, d_lambda, damp, st));
  }
  BA_CHECK(launch_schur_rhs(p, w->J_lin(), w->r_lin(), w->u, w->rhs, st, w->cam_pnt, w->tasks.pos));
  BA_CHECK(launch_prior_rhs(p, w->rhs, w->tasks.pos, st));  // - H'Lambda d of the camera and centre priors
  BA_CHECK(w->ldl.own_only ? comm_allreduce(p, w->rhs, w->npad, st) : reduce_camera_system(p, w, st, reduce32));
  if (normalize) BA_CHECK(scale_columns(p, w, lambda, d_lambda, st));
  // shared intrinsics (one rank, Float64, no column scaling, never recorded: all refused or excluded before): the bordered
  // solve.  From S_full: the border B = S_full E_g without its member rows, C and rhs_y; S and rhs masked in place to A and rhs_a
  const bool shared = p->grp_on();
  if (shared) {
    BA_CHECK(launch_border_prepare(p, &w->ldl, w->n, lambda, w->grp_row, w->grp_col, w->bord_B, w->rhs, w->bord_small, st));
    BA_HIP_CHECK(hipMemcpyAsync(w->bord_Y, w->bord_B, (size_t)(3 * p->grp_n) * w->npad * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  if (m.facto_f32) {  // round the assembled system to Float32, factor and solve there, widen the solution
    BA_CHECK(ensure_f32(w));
    if (!reduce32) BA_CHECK(launch_convert(w->ldl.S, w->ldl32.S, w->ldl.s_tiles * NB * NB, st));
    BA_CHECK(launch_convert(w->rhs, w->rhs32, w->npad, st));
    BA_CHECK(factor_solve<float>(p, &w->ldl32, w->rhs32, dist, st));
    BA_CHECK(launch_convert(w->rhs32, w->rhs, w->npad, st));
  } else {
    BA_CHECK(factor_solve<double>(p, &w->ldl, w->rhs, dist, st));
  }
  if (shared) {  // Y = A^-1 B in one pair of sweeps, then T = C - B'Y, y = T^-1 (rhs_y - B'a0) and the camera step a0 - Y y + E_g y
    BA_CHECK(dense_ldl_solve_multi<double>(p, &w->ldl, w->bord_Y, w->npad, 3 * p->grp_n, w->bord_w, st));
    BA_CHECK(launch_border_finish(p, &w->ldl, w->grp_col, w->bord_B, w->bord_Y, w->rhs, w->bord_small, st));
  }
  return step_from_solution(p, w, normalize, st);
}

// cr: the model value is |J delta + cr r|^2 (1 outside the line search)
// defer_delta: |delta_points|^2 and |delta_cameras|^2 are left to trial_point (one reduction pair with |r_trial|^2)
static int step_scalars(ba_problem *p, LMWork *w, hipStream_t st, double cr = -1.0, bool defer_delta = false) {
  const bool first = cr < 0;  // the step as linear_step left it (the line search calls with a rescaled delta and its own cr)
  if (first) cr = w->cr0();
  if (!(first && w->model_done)) BA_CHECK(launch_model_sq(p, w->J_lin(), w->r_lin(), w->delta, w->partial, w->scal, SH_MODEL, st, cr));
  w->model_done = false;
  if (!defer_delta) {
    // priors: their model term is added to SH_MODEL behind the observations' (with defer_delta: by trial_point, in one
    // kernel with the priors' cost at the trial point)
    BA_CHECK(launch_prior_step(p, w->delta, nullptr, st));
    SumsqJobs jobs;
    jobs.add(w->delta, 3 * p->npnts, w->scal, SH_DELTA_P);
    jobs.add(w->delta + 3 * p->npnts, w->n, w->scal_rep, RP_DELTA_C);
    if (p->pri_on()) jobs.add_sum(p->pri_model(), p->pri_total(), w->scal, SH_MODEL, true);
    BA_CHECK(launch_sumsq_multi(p, &jobs, w->partial_multi, st));
  }
  return BA_OK;
}

// with_delta: the step's two norms ride with |r_trial|^2 (step_scalars was told to leave them); recorded: the reduction
// also writes the controller's scalars and the pivot flag to the pinned host buffers
static int trial_point(ba_problem *p, LMWork *w, bool with_delta, bool recorded, hipStream_t st) {
  BA_CHECK(launch_axpy(p, w->nvar, w->x, w->delta, w->x_trial, st));
  if (w->mode.xf32) {  // x_suiv is a Float32 vector in the reference: round, evaluate in Float32
    BA_CHECK(launch_convert(w->x_trial, w->xf, w->nvar, st));
    BA_CHECK(launch_convert(w->xf, w->x_trial, w->nvar, st));
    BA_CHECK(launch_residual_f32(p, w->xf, w->rf, st));
    BA_CHECK(launch_convert(w->rf, w->r_trial, w->nequ, st));
  } else {
    BA_CHECK(launch_residual_f64(p, w->x_trial, w->r_trial, st));
    // per-observation information: the trial residual whitened in place, so the sums below (and, once the step is accepted,
    // refresh_linearisation) see r^
    BA_CHECK(launch_obs_scale(p, w->r_trial, nullptr, nullptr, nullptr, true, false, st));
  }
  const bool robust = p->loss != BA_LOSS_LINEAR;  // (the line search, the only caller without with_delta, is refused then)
  if (!with_delta && p->pri_on()) {  // (only the line search calls without with_delta, and ba_lm_solve refuses it with priors)
    ba_set_error("trial point of a rescaled step with priors (internal error: the line search is refused with priors)");
    return BA_ERR_ARG;
  }
  SumsqJobs jobs;
  if (with_delta) {
    jobs.add(w->delta, 3 * p->npnts, w->scal, SH_DELTA_P);
    jobs.add(w->delta + 3 * p->npnts, w->n, w->scal_rep, RP_DELTA_C);
  }
  if (robust) jobs.add_robust(w->r_trial, p->nobs, w->scal, SH_RSQ_TRIAL, p->loss, p->loss_scale * p->loss_scale);  // 2 f(x + delta)
  else jobs.add(w->r_trial, w->nequ, w->scal, SH_RSQ_TRIAL);
  if (p->pri_on()) {
    // the step's model term behind the observations' in SH_MODEL, 2 f_prior(x + delta) behind 2 f_obs in SH_RSQ_TRIAL (the
    // jobs of one launch are summed in order)
    BA_CHECK(launch_prior_step(p, w->delta, w->x_trial, st));
    jobs.add_sum(p->pri_model(), p->pri_total(), w->scal, SH_MODEL, true);
    jobs.add_sum(p->pri_cost_trial(), p->pri_total(), w->scal, SH_RSQ_TRIAL, true);
  }
  if (recorded) jobs.publish(w->scal, SH_COUNT, w->h_sh, w->scal_rep, RP_COUNT, w->h_rp, w->pivot_flag(), w->h_flag);
  return launch_sumsq_multi(p, &jobs, w->partial_multi, st);
}

// a factorisation's pivot flag (DenseLDLT::flag) as an error; zero_pivot_msg: what an exactly zero pivot means to this caller
static int pivot_flag_error(int h, const char *zero_pivot_msg = "reduced camera system: exactly zero pivot (SQDException in the reference)") {
  if (h == 2) {
    ba_set_error("dense factorisation: a hoisted diagonal tile never became ready (internal scheduling error)");
    return BA_ERR_HIP;
  }
  if (h) {
    ba_set_error("%s", zero_pivot_msg);
    return BA_ERR_ZERO_PIVOT;
  }
  return BA_OK;
}

// A hoisted diagonal kernel of the dense factorisation gave up waiting for its flag: the kernels were not running side by
// side (a counter-collecting profiler serialises them).  Switch the handle to the in-order schedule; the caller redoes
// the step (S was consumed by the abandoned factorisation).
static bool hoist_gave_up(LMWork *w) {
  if (*w->h_flag != 2 || (w->ldl.hoist_disabled && w->ldl32.hoist_disabled)) return false;
  w->ldl.hoist_disabled = w->ldl32.hoist_disabled = true;
  return true;
}

// a step body that ends with the pivot flag in w->h_flag and the stream synchronised: once more when hoist_gave_up
template <typename F>
static int with_hoist_retry(LMWork *w, F body) {
  BA_CHECK(body());
  if (hoist_gave_up(w)) BA_CHECK(body());
  return BA_OK;
}

// ---- recorded launch sequences ------------------------------------------------------------------------------------------
// what sequences recorded now would be recorded for (RecordedFor)
static RecordedFor recorded_for(ba_problem *p, LMWork *w) {
  const StepMode &m = w->mode;
  const int bits = m.normalize + 4 * (m.facto_f32 ? 1 : 0) + 8 * (m.xf32 ? 1 : 0) + 16 * p->loss + 128 * (p->fix_ncam > 0 ? 1 : 0) +
                   256 * (p->fix_npnt > 0 ? 1 : 0) + 512 * (p->info_on() ? 1 : 0);
  RecordedFor f;
  f.bits = bits;
  f.loss_scale = p->loss != BA_LOSS_LINEAR ? p->loss_scale : 1.0;
  f.d_fix_cam = p->d_fix_cam;
  f.d_fix_pnt = p->d_fix_pnt;
  if (p->info_on()) f.d_info = p->d_info, f.info_version = p->info_version;
  if (p->pri_on()) {
    for (int k = 0; k < PRI_KINDS; k++) {
      const PriorSet &q = p->pri[k];
      f.n_pri[k] = q.n;
      if (q.n > 0) f.d_pri[k][0] = q.idx, f.d_pri[k][1] = q.mu, f.d_pri[k][2] = q.info;
    }
    f.d_pri_work[0] = p->pri_d, f.d_pri_work[1] = p->pri_H, f.d_pri_work[2] = p->pri_val;
  }
  return f;
}
// are the recorded sequences those of the current handle state
static bool recorded_current(ba_problem *p, LMWork *w) { return w->rec.made_for == recorded_for(p, w); }

static bool graphs_allowed(ba_problem *p, LMWork *w) {
  if (w->rec.off || p->prof_on || p->comm.active() || w->mode.f16 || w->mode.pcg || p->grp_on()) return false;  // per-kernel events / communicator / Float16 path
  // the hoisted-diagonal schedule of large factorisations has a kernel wait for a flag raised by a kernel running
  // beside it: only with real streams is that concurrency certain (and the graphs gain nothing at that size)
  // (the block-sparse list schedule never hoists and is bound by its chain of short launches: recorded at any size)
  if (w->ldl.nt >= HOIST_MIN_TILES + 2 && !w->use_pattern) return false;  // (above HOIST_MAX_TILES graphs gain nothing either)
  return !env_off("BA_LM_GRAPH");
}

template <typename F>
static int record_graph(hipStream_t st, HipGraphExec *out, F body) {
  HipGraph g;
  BA_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  const int rc = body();
  const hipError_t e = hipStreamEndCapture(st, g.out());
  BA_CHECK(rc);
  BA_HIP_CHECK(e);
  BA_HIP_CHECK(hipGraphInstantiate(out->out(), g, nullptr, nullptr, 0));
  return BA_OK;
}

// replays the recorded form of `body` (recording it first when *g is empty) and waits for it.  Recording is an optimisation:
// when it fails the handle is marked off (plain launches from now on) and the caller issues the launches of `body` itself
template <typename F>
static int replay(LMWork *w, HipGraphExec *g, hipStream_t st, F body) {
  if (!*g && record_graph(st, g, body) != BA_OK) {
    (void)hipGetLastError();
    g->reset();
    w->rec.off = true;
    return BA_OK;
  }
  BA_HIP_CHECK(hipGraphLaunch(*g, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

// one trial step at damping `lambda`: linear solve, model decrease, trial residual, scalars and pivot flag to the host
static int trial_step(ba_problem *p, LMWork *w, double lambda, hipStream_t st) {
  auto launches = [&](double lam, bool recorded) -> int {
    BA_CHECK(linear_step(p, w, lam, recorded, st));
    BA_CHECK(step_scalars(p, w, st, -1.0, true));
    return trial_point(p, w, true, recorded, st);  // (recorded: + scalars and flag to the host)
  };
  if (graphs_allowed(p, w)) {
    if (!recorded_current(p, w)) {
      w->rec = RecordedSequences();  // (releases all four)
      w->rec.made_for = recorded_for(p, w);
    }
    if (w->mode.facto_f32) BA_CHECK(ensure_f32(w));  // no allocation while recording
    *w->h_lambda = lambda;  // read by the sequence's first kernel
    BA_CHECK(replay(w, &w->rec.step[w->parity], st, [&]() -> int { return launches(1.0, true); }));
    if (!w->rec.off) return BA_OK;  // (recorded sequences never hoist: graphs_allowed)
  }
  return with_hoist_retry(w, [&]() -> int {
    BA_CHECK(launches(lambda, false));
    BA_CHECK(comm_allreduce(p, w->scal + SH_TRIAL_FIRST, SH_TRIAL_COUNT, st));
    BA_HIP_CHECK(hipMemcpyAsync(w->h_flag, w->pivot_flag(), sizeof(int), hipMemcpyDeviceToHost, st));
    return fetch_scalars(p, w, st);  // (synchronises st)
  });
}

// after an accepted step (x/x_trial, r/r_trial already swapped): J, the normal-equation blocks, J'r, scalars to the host
static int accept_refresh(ba_problem *p, LMWork *w, hipStream_t st) {
  if (graphs_allowed(p, w)) {
    BA_CHECK(replay(w, &w->rec.refresh[w->parity], st, [&]() -> int {
      return refresh_linearisation(p, w, false, true, st);  // (+ scalars to the host)
    }));
    if (!w->rec.off) return BA_OK;
  }
  BA_CHECK(refresh_linearisation(p, w, false, false, st));
  return fetch_scalars(p, w, st);
}

// Recorded sequences only: the refresh after an accepted step and the NEXT trial step (its damping is known at the moment
// of acceptance) are submitted back to back and waited for once.  The host's work between two launches -- waking up from
// the wait, the accept test, submitting a sequence of ~110 nodes -- otherwise leaves the device idle twice per iteration
// (Dubrovnik: 31 + 79 us of a 3.0 ms iteration, LadyBug: the same of 0.44 ms; rocprofv3 kernel trace).  The refresh and the
// trial write disjoint scalar slots, so one read of the pinned buffers serves both.  If the stopping tests that need the
// refreshed |J'r| or |x| then end the loop, the prefetched step is dropped (never counted, x untouched).
static bool can_prefetch_trial(ba_problem *p, LMWork *w) {
  if (env_off("BA_LM_PREFETCH") || !graphs_allowed(p, w)) return false;  // read per call: a test compares both forms in one process
  return recorded_current(p, w) && w->rec.step[w->parity] && w->rec.refresh[w->parity];
}
static int accept_refresh_and_trial(LMWork *w, double lambda, hipStream_t st) {
  BA_HIP_CHECK(hipGraphLaunch(w->rec.refresh[w->parity], st));
  *w->h_lambda = lambda;  // read by the trial sequence's first kernel; the previous trial sequence has completed
  BA_HIP_CHECK(hipGraphLaunch(w->rec.step[w->parity], st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

// ---- the optional terms of the LM problem: robust loss, fixed parameters, priors, shared intrinsics, information --
// What the terms ask of an entry before its first launch: the uses of the handle a term is not carried through (TERM_RULES,
// check_terms), the device copies of their host tables (terms_upload), what a grouping asks of x (check_tied_x).
enum TermCond { TC_LINESEARCH, TC_X_F32, TC_FACTO_F32, TC_FACTO_F16, TC_NORMALIZE, TC_COMM, TC_COVARIANCE, TC_COUNT };
static const char *const TERM_COND_TEXT[TC_COUNT] = {
    "with linesearch = true",    "for a Float32 model (x_f32 = 1)", "with facto_type = Float32",       "with facto_type = Float16",
    "with normalize = :J or :A", "on a handle with a communicator", "by ba_covariance (clear it first)"};

struct TermUse {  // how an entry is about to use the handle
  const char *entry;
  bool linesearch = false, x_f32 = false, facto_f32 = false, facto_f16 = false, normalize = false, comm = false, covariance = false;
};

struct TermRule {  // a row of the matrix of DESIGN §5h
  const char *subject;             // the term and its setter, with the verb of the message
  bool (*on)(const ba_problem *);  // is the term set on the handle?
  TermCond refused[TC_COUNT + 1];  // the uses it is refused with, in the order they are reported; TC_COUNT ends the list
};

static const TermRule TERM_RULES[] = {
    {"a robust loss (ba_lm_set_loss) is", [](const ba_problem *p) { return p->loss != BA_LOSS_LINEAR; },
     {TC_LINESEARCH, TC_X_F32, TC_FACTO_F16, TC_COUNT}},
    {"fixed parameters (ba_lm_set_fixed) are", [](const ba_problem *p) { return p->fix_on(); }, {TC_FACTO_F16, TC_COUNT}},
    {"priors (ba_lm_set_priors) are", [](const ba_problem *p) { return p->pri_on(); },
     {TC_LINESEARCH, TC_X_F32, TC_FACTO_F16, TC_COMM, TC_COUNT}},
    {"shared intrinsics (ba_lm_set_shared_intrinsics) are", [](const ba_problem *p) { return p->grp_on(); },
     {TC_COMM, TC_X_F32, TC_FACTO_F32, TC_FACTO_F16, TC_NORMALIZE, TC_LINESEARCH, TC_COVARIANCE, TC_COUNT}},
    {"per-observation information (ba_lm_set_obs_info) is", [](const ba_problem *p) { return p->info_on(); },
     {TC_LINESEARCH, TC_X_F32, TC_FACTO_F16, TC_COMM, TC_COUNT}},
};

static int check_terms(const ba_problem *p, const TermUse &use) {
  const bool is[TC_COUNT] = {use.linesearch, use.x_f32, use.facto_f32, use.facto_f16, use.normalize, use.comm, use.covariance};
  for (const TermRule &t : TERM_RULES)
    for (const TermCond *c = t.refused; t.on(p) && *c != TC_COUNT; c++)
      if (is[*c]) {
        ba_set_error("%s: %s not supported %s", use.entry, t.subject, TERM_COND_TEXT[*c]);
        return BA_ERR_ARG;
      }
  return BA_OK;
}

int terms_upload(ba_problem *p) {
  BA_CHECK(fix_upload(p));
  BA_CHECK(prior_upload(p));
  BA_CHECK(shared_upload(p));
  return info_upload(p);
}

// what a grouping asks of x and of the mask (shared_check) on the camera part of x, fetched when x is on the device
static int check_tied_x(ba_problem *p, const double *x, bool x_on_device, const char *entry) {
  if (!p->grp_on()) return BA_OK;
  const double *xc = x + 3 * p->npnts;
  std::vector<double> host(x_on_device ? (size_t)(9 * p->ncams) : 0);
  if (x_on_device) {
    BA_HIP_CHECK(hipMemcpyAsync(host.data(), xc, host.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    BA_HIP_CHECK(hipStreamSynchronize(p->stream));
    xc = host.data();
  }
  return shared_check(p, xc, entry);
}

static int lm_step_impl(ba_problem *p, const double *x, double lambda, double *delta, double *half_sq_model,
                        double *jtr, bool facto_f32, bool pcg = false, double tol = 0, int max_iter = 0, int *cg_iters = nullptr) {
  if (!p || !x || !delta) {
    ba_set_error("ba_lm_step: null argument");
    return BA_ERR_ARG;
  }
  TermUse use{pcg ? "ba_lm_step_pcg" : facto_f32 ? "ba_lm_step_f32" : "ba_lm_step"};
  use.facto_f32 = facto_f32;
  use.comm = p->comm.active();
  BA_CHECK(check_terms(p, use));
  BA_CHECK(check_tied_x(p, x, false, use.entry));
  BA_HIP_CHECK(hipSetDevice(p->device));
  BA_CHECK(lm_ensure(p));
  BA_CHECK(terms_upload(p));
  LMWork *w = p->lm;
  hipStream_t st = p->stream;
  StepMode mode;
  mode.facto_f32 = facto_f32;
  mode.pcg = pcg;
  mode.pcg_tol = tol > 0 ? tol : 1e-8;
  mode.pcg_maxit = max_iter > 0 ? max_iter : 0;
  w->mode = mode;
  w->n_cg = 0;
  if (!pcg) BA_CHECK(ensure_dense(p, w));
  if (!pcg) BA_CHECK(ensure_shared_direct(p, w));
  BA_HIP_CHECK(hipMemcpyAsync(w->x, x, (size_t)w->nvar * sizeof(double), hipMemcpyHostToDevice, st));
  BA_CHECK(refresh_linearisation(p, w, true, false, st));
  // same fallback as the LM loop: a hoisted diagonal kernel that gave up -> in-order schedule, redo the step
  BA_CHECK(with_hoist_retry(w, [&]() -> int {
    BA_CHECK(linear_step(p, w, lambda, false, st));
    BA_HIP_CHECK(hipMemcpyAsync(w->h_flag, w->pivot_flag(), sizeof(int), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    return BA_OK;
  }));
  BA_CHECK(pivot_flag_error(*w->h_flag));
  BA_CHECK(step_scalars(p, w, st));
  BA_CHECK(comm_allreduce(p, w->scal + SH_TRIAL_FIRST, SH_TRIAL_COUNT, st));
  BA_CHECK(fetch_scalars(p, w, st));
  BA_HIP_CHECK(hipMemcpyAsync(delta, w->delta, (size_t)w->nvar * sizeof(double), hipMemcpyDeviceToHost, st));
  if (jtr) {
    BA_HIP_CHECK(hipMemcpyAsync(jtr, w->gp, (size_t)3 * p->npnts * sizeof(double), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipMemcpyAsync(jtr + 3 * p->npnts, w->gc, (size_t)w->n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BA_HIP_CHECK(hipStreamSynchronize(st));
  if (half_sq_model) *half_sq_model = 0.5 * w->h_sh[SH_MODEL];
  if (cg_iters) *cg_iters = (int)w->n_cg;
  return BA_OK;
}

extern "C" int ba_lm_schur_memory(ba_problem *p, int64_t *tiles_full, int64_t *tiles_held, int64_t *tiles_staging) {
  if (!p || !p->lm || !p->lm->ldl.S) {
    ba_set_error("ba_lm_schur_memory: no direct solve has run on this handle yet");
    return BA_ERR_ARG;
  }
  LMWork *w = p->lm;
  if (tiles_full) *tiles_full = w->ldl.nt * (w->ldl.nt + 1) / 2;
  if (tiles_held) *tiles_held = w->ldl.s_tiles;
  if (tiles_staging) *tiles_staging = w->ldl.own_only ? w->stage_tiles : 0;
  return BA_OK;
}

extern "C" int ba_lm_schur_pattern(ba_problem *p, double *tile_fill, double *flop_fill, int *sparse_schedule) {
  if (!p || !p->lm || !p->lm->ldl.S) {
    ba_set_error("ba_lm_schur_pattern: no direct solve has run on this handle yet");
    return BA_ERR_ARG;
  }
  LMWork *w = p->lm;
  if (tile_fill) *tile_fill = w->pattern.tile_fill;
  if (flop_fill) *flop_fill = w->pattern.flop_fill;
  if (sparse_schedule) *sparse_schedule = w->use_pattern ? 1 : 0;
  return BA_OK;
}

// (re)select the camera ordering of the handle; structures built under another one are dropped
static int set_ordering(ba_problem *p, int method) {
  if (method < 0 || method > 2) {
    ba_set_error("camera ordering: 0 (:AMD), 1 (:Metis) or 2 (the caller's numbering)");
    return BA_ERR_ARG;
  }
  BA_CHECK(lm_ensure(p));
  LMWork *w = p->lm;
  if (w->order_method == method) return BA_OK;
  if (w->ldl.S) {  // the task list, the pattern and the tiles depend on the order: start over
    lm_free(p);
    BA_CHECK(lm_ensure(p));
    w = p->lm;
  }
  w->order_method = method;
  return BA_OK;
}

extern "C" int ba_lm_set_ordering(ba_problem *p, int method) {
  if (!p) {
    ba_set_error("ba_lm_set_ordering: null handle");
    return BA_ERR_ARG;
  }
  BA_HIP_CHECK(hipSetDevice(p->device));
  return set_ordering(p, method);
}

extern "C" int ba_lm_schur_ordering(ba_problem *p, int64_t *perm1, const char **name) {
  if (!p || !p->lm || !p->lm->ldl.S) {
    ba_set_error("ba_lm_schur_ordering: no direct solve has run on this handle yet");
    return BA_ERR_ARG;
  }
  LMWork *w = p->lm;
  if (perm1)
    for (int64_t k = 0; k < p->ncams; k++) perm1[k] = (w->h_cam_perm.empty() ? k : (int64_t)w->h_cam_perm[(size_t)k]) + 1;
  if (name) *name = w->order_name;
  return BA_OK;
}

extern "C" int ba_lm_step_pcg(ba_problem *p, const double *x, double lambda, double tol, int max_iter, double *delta,
                              double *half_sq_model, double *jtr, int *cg_iters_out) {
  return lm_step_impl(p, x, lambda, delta, half_sq_model, jtr, false, true, tol, max_iter, cg_iters_out);
}

extern "C" int ba_lm_step(ba_problem *p, const double *x, double lambda, double *delta, double *half_sq_model,
                          double *jtr) {
  return lm_step_impl(p, x, lambda, delta, half_sq_model, jtr, false);
}

extern "C" int ba_lm_step_f32(ba_problem *p, const double *x, double lambda, double *delta, double *half_sq_model,
                              double *jtr) {
  return lm_step_impl(p, x, lambda, delta, half_sq_model, jtr, true);
}

// Covariance at x: Sigma = (J~_F' J~_F + sum_k H_k' Lambda_k H_k + lambda I)^-1 under the handle's loss, mask and priors, its cameras' 9 x 9 and points'
// 3 x 3 diagonal blocks.  The reduced camera system is assembled as linear_step does, with a damping vector that is 1 on the
// fixed entries and lambda on the free ones; its Float64 factor is inverted in place on the factor's pattern (selected
// inversion); the point blocks follow from the camera pairs that share a point.  Every buffer the next LM step reads is
// rebuilt by that step from its own x: the handle's later steps are unaffected.
extern "C" int ba_covariance(ba_problem *p, const double *x, double lambda, double rank_tol, double *cam_cov, double *pnt_cov,
                             double *min_rel_pivot) {
  if (!p || !x) {
    ba_set_error("ba_covariance: null argument");
    return BA_ERR_ARG;
  }
  if (!std::isfinite(lambda) || lambda < 0) {
    ba_set_error("ba_covariance: lambda must be finite and >= 0, got %g", lambda);
    return BA_ERR_ARG;
  }
  if (std::isnan(rank_tol)) {
    ba_set_error("ba_covariance: rank_tol is NaN (< 0: the default 1e-10, 0: no rank check)");
    return BA_ERR_ARG;
  }
  if (p->comm.active()) {
    ba_set_error("ba_covariance: one rank only (a communicator is attached to this handle)");
    return BA_ERR_ARG;
  }
  TermUse use{"ba_covariance"};
  use.covariance = true;
  BA_CHECK(check_terms(p, use));
  const double tol = rank_tol < 0 ? 1e-10 : rank_tol;
  BA_HIP_CHECK(hipSetDevice(p->device));
  BA_CHECK(lm_ensure(p));
  BA_CHECK(terms_upload(p));
  LMWork *w = p->lm;
  hipStream_t st = p->stream;
  w->mode = StepMode();
  BA_CHECK(ensure_dense(p, w));
  const int64_t np3 = 3 * p->npnts;
  std::vector<double> hdamp((size_t)w->nvar, lambda);
  for (int64_t j = 0; j < p->npnts && p->fix_npnt > 0; j++)
    if (p->h_fix_pnt[(size_t)j])
      for (int q = 0; q < 3; q++) hdamp[(size_t)(3 * j + q)] = 1.0;
  for (int64_t c = 0; c < p->ncams && p->fix_ncam > 0; c++)
    for (int b = 0; b < 9; b++)
      if ((p->h_fix_cam[(size_t)c] >> b) & 1u) hdamp[(size_t)(np3 + 9 * c + b)] = 1.0;
  DevBuf<double> damp, sdiag, ratio, part, cams, pnts;
  DevBuf<int> iota;
  BA_CHECK(upload(damp, hdamp));
  BA_CHECK(sdiag.alloc(w->npad));
  BA_CHECK(ratio.alloc(1));
  BA_HIP_CHECK(hipMemcpyAsync(w->x, x, (size_t)w->nvar * sizeof(double), hipMemcpyHostToDevice, st));
  BA_CHECK(refresh_linearisation(p, w, true, false, st));
  BA_CHECK(with_hoist_retry(w, [&]() -> int {  // as lm_step_impl: the in-order schedule, the factorisation again
    BA_CHECK(launch_schur_prep(p, lambda, w->Hpp, w->gp, w->Uinv, w->u, st, nullptr, damp));
    BA_CHECK(assemble_local(p, w, lambda, nullptr, damp, st));  // (one rank: lam_diag = lambda)
    BA_CHECK(launch_cov_sdiag(p, &w->ldl, w->n, sdiag, nullptr, false, st));
    BA_CHECK(dense_ldl_factor(p, &w->ldl, st, (double *)nullptr));
    BA_HIP_CHECK(hipMemcpyAsync(w->h_flag, w->pivot_flag(), sizeof(int), hipMemcpyDeviceToHost, st));
    BA_HIP_CHECK(hipStreamSynchronize(st));
    return BA_OK;
  }));
  BA_CHECK(pivot_flag_error(*w->h_flag, "ba_covariance: exactly zero pivot in the reduced camera system (fix a gauge, or pass lambda > 0)"));
  double h_ratio = 0;
  BA_CHECK(launch_cov_sdiag(p, &w->ldl, w->n, sdiag, ratio, true, st));
  BA_HIP_CHECK(hipMemcpyAsync(&h_ratio, ratio, sizeof(double), hipMemcpyDeviceToHost, st));
  BA_HIP_CHECK(hipStreamSynchronize(st));
  if (min_rel_pivot) *min_rel_pivot = h_ratio;
  if (tol > 0 && !(h_ratio > tol)) {
    ba_set_error("ba_covariance: the reduced camera system is numerically singular (min pivot / diagonal = %.3g <= rank_tol = %.3g): "
                 "fix a gauge (ba_lm_set_fixed: e.g. one camera's pose and one translation component of another) or pass "
                 "lambda > 0", h_ratio, tol);
    return BA_ERR_ZERO_PIVOT;
  }
  if (!cam_cov && !pnt_cov) return BA_OK;
  std::vector<int> h_iota((size_t)w->ldl.nt);
  for (int64_t k = 0; k < w->ldl.nt; k++) h_iota[(size_t)k] = (int)k;
  BA_CHECK(upload(iota, h_iota));
  BA_CHECK(part.alloc(cov_part_tiles(w->ldl.nt) * NB * NB));
  BA_CHECK(dense_ldl_selinv(p, &w->ldl, iota, part, st));
  const uint16_t *fc = p->fix_ncam > 0 ? (const uint16_t *)p->d_fix_cam : nullptr;
  const uint8_t *fp = p->fix_npnt > 0 ? (const uint8_t *)p->d_fix_pnt : nullptr;
  if (cam_cov) {
    BA_CHECK(cams.alloc(81 * p->ncams));
    BA_CHECK(launch_cov_cams(p, &w->ldl, w->tasks.pos, fc, cams, st));
    BA_HIP_CHECK(hipMemcpyAsync(cam_cov, cams, (size_t)81 * p->ncams * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (pnt_cov) {
    BA_CHECK(pnts.alloc(9 * p->npnts));
    BA_CHECK(launch_cov_points(p, &w->ldl, w->tasks.pos, w->J, w->Yobs, w->Uinv, fp, pnts, st));
    BA_HIP_CHECK(hipMemcpyAsync(pnt_cov, pnts, (size_t)9 * p->npnts * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return BA_OK;
}

// the option combinations ba_lm_solve refuses: the options among themselves, then the terms on the handle (check_terms)
static int check_solve_opts(const ba_problem *p, const ba_lm_opts *o) {
  if (o->variant != 0 && o->variant != 1) {
    ba_set_error("ba_lm_solve: variant must be 0 (LevenbergMarquardt.jl) or 1 (lm.jl)");
    return BA_ERR_ARG;
  }
  if (o->facto < 0 || o->facto > 2) {
    ba_set_error("ba_lm_solve: facto must be 0 (:LDL), 1 (:QR) or 2 (:PCG)");
    return BA_ERR_ARG;
  }
  if (o->facto == 2 && o->facto_type == 2) {
    ba_set_error("ba_lm_solve: facto = :PCG runs in Float64 (facto_type = Float16 belongs to the :LDL branch)");
    return BA_ERR_ARG;
  }
  if (o->facto == 2 && o->normalize != 0) {
    ba_set_error("ba_lm_solve: facto = :PCG has its own scaling (block-Jacobi preconditioner): normalize must be :None");
    return BA_ERR_ARG;
  }
  if (o->facto == 2 && o->facto_type == 1 && !o->x_f32) {
    ba_set_error("ba_lm_solve: facto = :PCG runs in Float64; facto_type = Float32 belongs to the direct branches "
                 "(for a Float32 model it is the default and is ignored by :PCG)");
    return BA_ERR_ARG;
  }
  if (o->facto_type < 0 || o->facto_type > 2) {
    ba_set_error("ba_lm_solve: facto_type must be 0 (eltype(x)), 1 (Float32) or 2 (Float16)");
    return BA_ERR_ARG;
  }
  if (o->facto_type == 2 && (o->variant != 1 || o->facto != 0 || p->comm.active())) {
    ba_set_error("ba_lm_solve: facto_type = Float16 exists in lm.jl's :LDL branch only (src/lm.jl:92-95,165-169), one GPU");
    return BA_ERR_ARG;
  }
  if (o->normalize < 0 || o->normalize > 2) {
    ba_set_error("ba_lm_solve: normalize must be 0 (:None), 1 (:J) or 2 (:A)");
    return BA_ERR_ARG;
  }
  if (o->perm < 0 || o->perm > 2) {
    ba_set_error("ba_lm_solve: perm must be 0 (:AMD), 1 (:Metis) or 2 (the caller's camera numbering)");
    return BA_ERR_ARG;
  }
  TermUse use{"ba_lm_solve"};
  use.linesearch = o->variant == 1 && o->linesearch;
  use.x_f32 = o->x_f32 != 0;
  use.facto_f32 = o->variant == 1 && o->facto_type == 1;
  use.facto_f16 = o->variant == 1 && o->facto_type == 2;
  use.normalize = o->normalize != 0;
  use.comm = p->comm.active();
  return check_terms(p, use);
}

static int lm_solve_impl(ba_problem *p, const ba_lm_opts *o, double *x_inout, bool x_on_device, ba_lm_stats *stats, ba_log_cb cb,
                         void *cb_ctx) {
  if (!p || !o || !x_inout || !stats) {
    ba_set_error("ba_lm_solve: null argument");
    return BA_ERR_ARG;
  }
  BA_CHECK(check_solve_opts(p, o));
  BA_HIP_CHECK(hipSetDevice(p->device));
  const double t_start = wall();
  BA_CHECK(set_ordering(p, o->perm));  // (lm_ensure inside)
  BA_CHECK(terms_upload(p));
  BA_CHECK(check_tied_x(p, x_inout, x_on_device, "ba_lm_solve"));  // the members of a group must enter bit-identical
  LMWork *w = p->lm;
  hipStream_t st = p->stream;
  const int V = o->variant;
  const bool xf32 = o->x_f32 != 0;  // eltype(x) = Float32: Float32 iterates and evaluations
  StepMode mode;
  mode.normalize = o->normalize;
  mode.xf32 = xf32;
  mode.f16 = V && o->facto_type == 2;
  mode.facto_f32 = V && o->facto_type >= 1 && o->facto != 2;  // Float16 inputs are eliminated and factored in Float32
  mode.pcg = o->facto == 2;
  mode.pcg_tol = o->pcg_tol > 0 ? o->pcg_tol : 1e-8;
  mode.pcg_maxit = o->pcg_max_iter > 0 ? o->pcg_max_iter : 0;
  w->mode = mode;
  if (xf32) BA_CHECK(ensure_xf32(p, w));
  if (mode.f16) BA_CHECK(ensure_f16(p, w));
  w->n_cg = 0;
  if (!mode.pcg) BA_CHECK(ensure_dense(p, w));  // (here, not in linear_step: no allocation while a graph is being recorded)
  if (!mode.pcg) BA_CHECK(ensure_shared_direct(p, w));

  memset(stats, 0, sizeof *stats);
  stats->status = BA_ST_UNKNOWN;
  double *h_sh = w->h_sh, *h_rp = w->h_rp;

  BA_HIP_CHECK(hipMemcpyAsync(w->x, x_inout, (size_t)w->nvar * sizeof(double), x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (xf32) {  // x0 is a Float32 vector at the reference's boundary; make sure of it
    BA_CHECK(launch_convert(w->x, w->xf, w->nvar, st));
    BA_CHECK(launch_convert(w->xf, w->x, w->nvar, st));
  }
  BA_CHECK(refresh_linearisation(p, w, true, false, st));  // r, J, J'r   (lm.jl:39-58)
  BA_CHECK(fetch_scalars(p, w, st));
  stats->n_residual++;
  stats->n_jacobian++;
  // the scalar side of the solve: every decision below is the controller's (ba_lm_controller.h), from the sums the device
  // publishes; this loop submits the work and hands them over
  LMController c(*o, p->loss != BA_LOSS_LINEAR, w->cr0());
  auto sums = [&] {
    return LMSums{h_sh[SH_RSQ], h_sh[SH_RTSQ], h_sh[SH_GP] + h_rp[RP_GC], h_sh[SH_X_P] + h_rp[RP_X_C], h_sh[SH_MODEL], h_sh[SH_RSQ_TRIAL],
                  h_sh[SH_DELTA_P] + h_rp[RP_DELTA_C]};
  };
  auto emit = [&] {  // one log row, the reference's columns: to the caller's callback and, verbose, to stderr
    const LMRow r = c.row();
    if (cb) cb(cb_ctx, r.iter, r.f, r.df, r.norm_jtr, r.lambda, r.norm_delta, r.rho, r.accepted);
    if (o->verbose)
      fprintf(stderr, "%6d %14.7e %10.2e %10.2e %10.2e %10.2e %10.2e %s\n", r.iter, r.f, r.df, r.norm_jtr, r.lambda, r.norm_delta, r.rho,
              V ? (r.accepted ? "acc" : "rej") : (r.accepted ? "true" : "false"));
  };
  // every parameter fixed (ba_lm_set_fixed): nothing to solve for.  The cameras' mask is the same on every rank; the points are
  // counted over the ranks.
  bool all_fixed = false;
  if (p->fix_ncam == 9 * p->ncams) {
    double free_pts = (double)(p->npnts - p->fix_npnt);
    if (p->comm.active()) {
      BA_HIP_CHECK(hipMemcpyAsync(w->partial, &free_pts, sizeof(double), hipMemcpyHostToDevice, st));
      BA_CHECK(comm_allreduce(p, w->partial, 1, st));
      BA_HIP_CHECK(hipMemcpyAsync(&free_pts, w->partial, sizeof(double), hipMemcpyDeviceToHost, st));
      BA_HIP_CHECK(hipStreamSynchronize(st));
    }
    all_fixed = free_pts == 0;
  }
  c.start(sums(), all_fixed);
  bool have_trial = false;
  int rc = BA_OK;
  const double t_loop = wall();

  while (!c.done()) {
    c.begin_iteration();
    if (!V) emit();                      // LevenbergMarquardt.jl:143-147
    if (have_trial) have_trial = false;  // submitted with the refresh of the step accepted last (accept_refresh_and_trial)
    else if ((rc = trial_step(p, w, c.lambda(), st)) != BA_OK) break;  // lm.jl:154-254
    stats->n_factor++;
    stats->n_residual++;
    if ((rc = pivot_flag_error(*w->h_flag)) != BA_OK) break;
    c.judge(sums());
    while (c.wants_halving()) {  // lm.jl:264-295
      const LMController::Halving h = c.halve();
      if ((rc = launch_scale_scalar(p, w->nvar, w->delta, h.scale, st)) != BA_OK) break;
      if ((rc = step_scalars(p, w, st, h.c_r)) != BA_OK) break;
      if ((rc = trial_point(p, w, false, false, st)) != BA_OK) break;
      stats->n_residual++;
      if ((rc = comm_allreduce(p, w->scal + SH_TRIAL_FIRST, SH_TRIAL_COUNT, st)) != BA_OK) break;
      if ((rc = fetch_scalars(p, w, st)) != BA_OK) break;
      c.judge(sums());
    }
    if (rc != BA_OK) break;
    if (!c.step_norm(sums())) continue;  // NaN step: the loop ends, status :exception (lm.jl:297-302)
    if (V) emit();                       // lm.jl:304

    if (!c.accepted()) {
      stats->n_rejected++;
      c.reject();
    } else {
      stats->n_accepted++;
      // (what of the stopping tests is known before the refresh decides whether the next trial step goes out with it)
      const bool stop_known = c.accept();
      std::swap(w->x, w->x_trial);  // x .= x_suiv
      std::swap(w->r, w->r_trial);  // r .= r_suiv
      w->parity ^= 1;
      if (!stop_known && can_prefetch_trial(p, w)) {
        if ((rc = accept_refresh_and_trial(w, c.lambda(), st)) != BA_OK) break;
        have_trial = true;
      } else if ((rc = accept_refresh(p, w, st)) != BA_OK) break;  // J, J'r  (lm.jl:341,370)
      stats->n_jacobian++;
      c.refreshed(sums());
    }
    c.end_iteration();
  }
  if (rc == BA_OK && !V) emit();  // LevenbergMarquardt.jl:368
  stats->loop_s = wall() - t_loop;

  stats->status = rc != BA_OK ? BA_ST_EXCEPTION : c.status();
  stats->iter = c.iter();
  stats->objective = c.objective();
  stats->dual_feas = c.dual_feas();
  stats->lambda_final = c.lambda();
  stats->n_cg = (int)w->n_cg;
  {
    hipError_t e = hipMemcpyAsync(x_inout, w->x, (size_t)w->nvar * sizeof(double), x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == BA_OK) {
      ba_set_error("solution copy: %s", hipGetErrorString(e));
      rc = BA_ERR_HIP;
    }
  }
  stats->elapsed_s = wall() - t_start;
  return rc;  // a NaN step is not an error of the call: status :exception, as in the reference (lm.jl:297-302,401-402)
}

extern "C" int ba_lm_solve(ba_problem *p, const ba_lm_opts *o, double *x_inout, ba_lm_stats *stats, ba_log_cb cb,
                           void *cb_ctx) {
  return lm_solve_impl(p, o, x_inout, false, stats, cb, cb_ctx);
}

extern "C" int ba_lm_solve_dev(ba_problem *p, const ba_lm_opts *o, double *d_x_inout, ba_lm_stats *stats, ba_log_cb cb,
                               void *cb_ctx) {
  return lm_solve_impl(p, o, d_x_inout, true, stats, cb, cb_ctx);
}
