// Internal declarations shared by the translation units of libba_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../../include/ba_hip.h"
#include "ba_order.h"  // TilePattern, camera orderings (host only)

void ba_set_error(const char *fmt, ...);
#include "ba_launch.h"  // BA_LAUNCH: every kernel launch; grid_for

#define BA_HIP_CHECK(expr)                                                                          \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) {                                                                         \
      ba_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));            \
      return BA_ERR_HIP;                                                                            \
    }                                                                                               \
  } while (0)

#define BA_CHECK(expr)            \
  do {                            \
    int _rc = (expr);             \
    if (_rc != BA_OK) return _rc; \
  } while (0)

// environment switches: env_off -- the variable is set to a value starting with '0'; env_int -- its value, or
// dflt when it is not set
inline bool env_off(const char *name) {
  const char *e = getenv(name);
  return e && e[0] == '0';
}
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ---- owners of device resources -------------------------------------------------------------------------------------------
// Every device buffer, pinned host buffer, stream, event and graph the library creates is held by one of these and released
// by it: when the owner is destroyed, reset, moved onto or filled again.  They are the only code that creates or releases
// such a resource (tests/test_host.py).  Move-only; an owner converts to its raw handle, so launch sites and pointer
// arithmetic read as with the raw one.  Views into an owner's memory stay raw pointers.  Release needs the handle's device
// to be current: every path into a teardown sets it.
template <typename H, hipError_t (*Release)(H)>
class Owner {
 public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h_(o.release()) {}
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.release();
    }
    return *this;
  }
  ~Owner() { reset(); }
  void reset() {
    if (h_) (void)Release(h_);
    h_ = nullptr;
  }
  H release() {  // the caller takes the handle over
    H h = h_;
    h_ = nullptr;
    return h;
  }
  H *out() {  // for a call that creates the handle in place
    reset();
    return &h_;
  }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};

template <typename T>
hipError_t free_dev(T *p) { return hipFree(p); }
template <typename T>
hipError_t free_pinned(T *p) { return hipHostFree(p); }

// n elements of T in device memory, or (Pinned) in pinned host memory the device can address; n <= 0 allocates one
template <typename T, bool Pinned = false>
class Buf : public Owner<T *, Pinned ? free_pinned<T> : free_dev<T>> {
 public:
  int alloc(int64_t n) {
    const size_t bytes = (size_t)(n > 0 ? n : 1) * sizeof(T);
    if (Pinned) BA_HIP_CHECK(hipHostMalloc((void **)this->out(), bytes));
    else BA_HIP_CHECK(hipMalloc((void **)this->out(), bytes));
    return BA_OK;
  }
};
template <typename T>
using DevBuf = Buf<T>;
template <typename T>
using PinnedBuf = Buf<T, true>;

class HipStream : public Owner<hipStream_t, hipStreamDestroy> {
 public:
  int create(unsigned flags) {
    BA_HIP_CHECK(hipStreamCreateWithFlags(out(), flags));
    return BA_OK;
  }
  int create(unsigned flags, int priority) {
    BA_HIP_CHECK(hipStreamCreateWithPriority(out(), flags, priority));
    return BA_OK;
  }
};
class HipEvent : public Owner<hipEvent_t, hipEventDestroy> {
 public:
  int create(unsigned flags = hipEventDefault) {
    BA_HIP_CHECK(hipEventCreateWithFlags(out(), flags));
    return BA_OK;
  }
};
using HipGraph = Owner<hipGraph_t, hipGraphDestroy>;
using HipGraphExec = Owner<hipGraphExec_t, hipGraphExecDestroy>;

// d <- a new device buffer of h.size() + extra elements (at least one) that starts with h
template <typename T>
int upload(DevBuf<T> &d, const std::vector<T> &h, size_t extra = 0) {
  BA_CHECK(d.alloc((int64_t)(h.size() + extra)));
  if (!h.empty()) BA_HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return BA_OK;
}

// ---- dense reduced-camera system ------------------------------------------------------------------
// S is stored as the lower block triangle of NB x NB tiles, each tile contiguous row-major (128 KiB).  Tile (i,j),
// j <= i, sits at tile index col_off[j] + (i - j): a tile column is contiguous (rows j..nt-1).  Tile columns are taken
// in PAIRS (2q, 2q+1) -- the unit the factorisation works in -- and the pairs are grouped by owner rank q mod world
// (ascending q inside a group), so that the part of S a rank owns in the distributed factorisation is ONE contiguous
// range (a single reduce onto its owner per rank).  With world == 1 this is plain column order.
constexpr int NB = 128;
// Tile (i, j), j <= i, of the packed reduced camera matrix sits at tile offset tix(col_off, i, j).  col_off points ONE PAST the
// head of its table: col_off[-1] = 0 for the dense layout (a tile column is contiguous: col_off[j] + (i - j)), or = nt for the
// compressed layout of a block-sparse pattern, where col_off[nt + i nt + j] is the position of tile row i among the stored
// rows of column j (negative, and so a negative result, for a tile outside the pattern: nothing is allocated for it).
// Enumeration of the lower triangle of an m x m tile grid in SUPER-BLOCKS of TSB x TSB tiles (block rows top to bottom, blocks
// left to right, row-major inside a block; the diagonal blocks hold their lower triangle): t -> (ii, jj), jj <= ii.  The
// workgroups of the bulk trailing update that run at the same time (consecutive t) then share TSB row panels of each
// operand instead of one panel of A and one panel PER TILE of B -- the operand reads that miss the XCD's L2 drop by ~TSB / 2.
// t = 0, 1, 2 are (0,0), (1,0), (1,1): what the hoisted diagonal kernels wait for.
constexpr int TSB = 8;
__host__ __device__ inline void tri_blocked(int t, int m, int *ii, int *jj, int sb = TSB) {
  // tiles before block row bi (all block rows above it are full): sum_{r < bi} (sb^2 r + sb (sb + 1) / 2)
  const int full = sb * sb, tri = sb * (sb + 1) / 2;
  int lo = 0, hi = (m + sb - 1) / sb;  // largest bi with start(bi) <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (full * mid * (mid - 1) / 2 + tri * mid <= t) lo = mid;
    else hi = mid;
  }
  const int bi = lo;
  int rem = t - (full * bi * (bi - 1) / 2 + tri * bi);
  const int h = (m - sb * bi) < sb ? (m - sb * bi) : sb;  // tile rows in this block row
  if (rem < bi * sb * h) {
    const int bj = rem / (sb * h), r2 = rem - bj * (sb * h);
    *ii = sb * bi + r2 / sb;
    *jj = sb * bj + r2 % sb;
  } else {
    rem -= bi * sb * h;
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= rem) r++;
    *ii = sb * bi + r;
    *jj = sb * bi + rem - r * (r + 1) / 2;
  }
}

// Tickets of the bulk pair update (k_ldl_update, plain dense form): its persistent workgroups draw the launch's nblk tiles
// (indices of the enumeration above) from nine counters -- one queue per XCD, which covers the contiguous range of
// per = ceil(nblk / 8) tiles that the static chunked map gives the blocks of one XCD, and the first-come counter
// TICKET_READY for the first ready_tiles tiles (what a hoisted workgroup waits for; taken off queue 0's range).  The n-th
// draw (n = the counter's value before its fetch_add) from source src is tile ticket_tile(...), or -1: that source is empty.
// Every tile belongs to exactly one source and one n, so each is handed out once whatever the order of the draws.
constexpr int TICKET_QUEUES = 8, TICKET_READY = TICKET_QUEUES;
constexpr int TICKET_SLOTS = 16;  // ints per launch: the nine counters, padded to a 64-byte line
__host__ __device__ inline int ticket_tile(int nblk, int ready_tiles, int src, int n) {
  const int nready = ready_tiles < nblk ? ready_tiles : nblk;
  if (src == TICKET_READY) return n < nready ? n : -1;
  const int per = (nblk + TICKET_QUEUES - 1) / TICKET_QUEUES;
  const int lo = src * per > nready ? src * per : nready;
  const int hi = (src + 1) * per < nblk ? (src + 1) * per : nblk;
  return n < hi - lo ? lo + n : -1;
}
// the sources a workgroup on XCD xcd draws from, in order: s = 0 the ready counter, then its own queue, then the others cyclically
__host__ __device__ inline int ticket_source(int xcd, int s) { return s == 0 ? TICKET_READY : (xcd + s - 1) % TICKET_QUEUES; }

__host__ __device__ inline int64_t tix(const int64_t *__restrict__ col_off, int64_t i, int64_t j) {
  const int64_t n = col_off[-1];
  return col_off[j] + (n ? col_off[n + i * n + j] : (i - j));
}
constexpr int64_t BA_NO_TILE = -((int64_t)1 << 40);
// host: fill col_off (nt entries) and, when own_range != null, the [begin, end) tile ranges of the `world` owners
void dense_ldl_layout(int64_t nt, int world, std::vector<int64_t> *col_off, std::vector<int64_t> *own_range);

enum ProfClass {
  PC_RESIDUAL = 0,
  PC_JAC_STRUCTURE,
  PC_JAC_COORD,
  PC_POINT_BLOCKS,
  PC_CAM_BLOCKS,
  PC_SCHUR_PREP,
  PC_SCHUR_S,
  PC_SCHUR_RHS,
  PC_LDL_DIAG,
  PC_LDL_TRSM,
  PC_LDL_SYRK,    // update of the next tile column inside a panel pair (k_ldl_col_rs)
  PC_LDL_UPDATE,  // bulk pair update of the trailing matrix (k_ldl_update)
  PC_LDL_UPDATE_RS,  // short pair updates in row-split form (k_ldl_update_rs)
  PC_SOLVE,
  PC_BACKSUB,
  PC_TRIAL,
  PC_REDUCE,
  PC_COMM,
  PC_ROBUST,  // "k_robust_scale": k_obs_scale on a handle without information (robust loss: reweighting of r and J)
  PC_FIXED,   // k_fix_mask (fixed parameters: zeroing of their columns of J)
  PC_COV_INV,     // covariance (ba_covariance): selected inversion of the factored S, with the rank check's diag(S) and min D_i / S_ii
  PC_COV_CAMS,    // covariance: the cameras' 9 x 9 blocks (k_cov_cams)
  PC_COV_POINTS,  // covariance: the points' 3 x 3 blocks (k_cov_points)
  PC_PRIOR,       // Gaussian priors (ba_lm_set_priors): k_prior_*_lin at a linearisation, k_prior_*_rhs per linear step, k_prior_*_step per trial step
  PC_SHARED_BORDER,  // shared intrinsics (ba_lm_set_shared_intrinsics): the border product S E_g, its E' reductions, the masking of S and the E' reductions / expansions of vectors
  PC_SHARED_SWEEP,   // shared intrinsics: the multi-right-hand-side triangular sweeps (k_fwd_step / k_bwd_step with grid.y = the number of columns; also ba_dense_ldl_solve_multi)
  PC_SHARED_SMALL,   // shared intrinsics: T = C - B'Y and the 3G x 3G Cholesky solve fused with the update of the camera step
  PC_INFO,           // per-observation information (ba_lm_set_obs_info): "k_info_whiten": k_obs_scale on a handle with it, the whitening of r and J (with the loss's reweighting)
  PC_REFINE_POINTS,  // points with the cameras held (ba_refine_points): k_cam_pre and k_refine_points
  PC_REFINE_CAMERAS,  // cameras with the points held (ba_refine_cameras): k_refine_cameras
  PC_RESECT_CAMERAS,  // linear resection before it (ba_resect_cameras): k_resect_cameras
  PC_RANSAC_CAMERAS,  // consensus stage before that (ba_ransac_cameras): k_ransac_hypotheses, _select, _rescore, _mask_info
  PC_RANSAC_POINTS,   // consensus stage before the triangulation (ba_ransac_points): k_cam_pre, k_ransac_points, k_ransac_mask_info
  PC_HOMOGRAPHY,      // homography of camera pairs (ba_homography): k_pair_rays, k_pair_hypotheses_h, k_pair_select_h, k_pair_fit_h
  PC_ROTAVG,          // "k_rotation_averaging" (ba_rotation_loops, ba_average_rotations): k_rotation_loops, k_rotavg_sweep, k_rotavg_edges, k_rotavg_sum, k_rotavg_finish
  PC_TRANSAVG,        // "k_translation_averaging" (ba_translation_loops, ba_average_translations): every kernel of ba_transavg_kernels.hip
  PC_SIMILARITY,        // "k_similarity" (ba_similarity): k_similarity_hypotheses, k_similarity_select, k_similarity_fit
  PC_COUNT
};
extern const char *const kProfNames[PC_COUNT];

struct ProfSlot {
  double ms = 0;
  int64_t calls = 0;
};

template <typename T>
struct DenseLDLT {  // workspace of the blocked LDL^T in scalar type T, n = 9*ncams padded to nt*NB
  int64_t n = 0, nt = 0;
  DevBuf<T> S;             // packed lower tiles
  DevBuf<T> V;             // 8 x nt tiles: V_i = L_ik * D_k, (two runs) x (two slots, alternating for the look-ahead) x two panels
  T *vpanel(int slot, int j, int run = 0) { return V + (int64_t)(4 * run + 2 * slot + j) * nt * NB * NB; }  // panel j of a pair
  DevBuf<T> Linv;          // nt tiles: inverse of each unit-lower diagonal tile
  DevBuf<T> D;             // nt*NB pivots (+ nt*NB scratch)
  int64_t *col_off = nullptr;           // device: tile column offsets (see tix)
  std::vector<int64_t> h_col_tab;       // host copy of the table: [head | nt column offsets | (compressed) nt x nt row positions]
  DevBuf<int64_t> col_tab;              // the device allocation (col_off = col_tab + 1)
  const int64_t *hco() const { return h_col_tab.data() + 1; }
  int64_t *hco() { return h_col_tab.data() + 1; }
  std::vector<int64_t> own_range;       // world + 1 tile offsets: rank r owns tiles [own_range[r], own_range[r+1])
  int world = 1, rank = 0;              // distribution of the tile column pairs (owner of pair q: q % world)
  std::vector<int> h_own_cols;          // tile columns owned by this rank, ascending
  std::vector<int64_t> h_own_pref;      // h_own_pref[m] = tiles in the owned columns before h_own_cols[m]
  DevBuf<int> own_cols;                 // device copies
  DevBuf<int64_t> own_pref;
  DevBuf<double> flag_sum;              // device double: the pivot flag on its way through the all-reduce
  DevBuf<int> flag;        // device int: set to 1 on an exactly zero pivot (2: a hoisted diagonal tile never became ready)
  DevBuf<int> ready;       // nt device ints: tile (k,k) has received its last trailing update (hoisted-diagonal schedule)
  DevBuf<int> tickets;     // TICKET_SLOTS ints per tile column pair: the counters of its ticketed pair update (ticket_tile)
  int wg_slots = 0;        // workgroups of k_ldl_update the device holds at once (two per CU): grid of a ticketed launch
  HipStream hoist;               // second stream of the hoisted-diagonal schedule (no CU mask)
  HipStream rest;                // look-ahead of the block-sparse schedule: the rest of a pair's update (lowest priority)
  HipEvent ev_top;
  bool hoist_disabled = false;   // a hoisted kernel once timed out (kernels serialised by a profiler): never again on this handle
  bool hoisting = false;         // the factorisation forks onto `hoist` (set by dense_ldl_factor's schedule choice)
  HipEvent ev_chain;              // recorded behind each hoisted diagonal kernel
  // distributed factorisation with look-ahead: panels of pair q received (transfer stream), update of pair q launched
  HipEvent ev_recv[2], ev_upd[2];
  // per-rank ownership of S (distributed factorisation): S holds this rank's tile columns only (s_tiles tiles), col_off /
  // hco() are rank-local offsets (negative for other ranks' columns), h_glob_off the owner-major global layout;
  // Lb: L = V D^-1 of the panel pairs in flight (the layout of V), bpart: partial products of the backward sweep
  bool own_only = false;
  int64_t s_tiles = 0;
  std::vector<int64_t> h_glob_off;
  DevBuf<T> Lb, bpart;
  T *L_of(const T *v) { return Lb + (v - V); }  // the L buffer that travels with panel buffer v of V
  // block-sparse S (one GPU): the pattern's row / column lists on the device; null pattern = dense
  bool sparse = false;
  const TilePattern *pat = nullptr;
  DevBuf<int> prow, lcol, lpair;
  // ... on several ranks (per-rank ownership of the PATTERN's tile columns): tiles stored per tile column, and per tile column
  // pair q the tiles (i, j) -- both in U_q, j owned by this rank, sorted by (j, i) -- its trailing update touches here; the first
  // h_upd_lead[q] of them lie in the next pair's own tile columns (look-ahead of the distributed factorisation)
  std::vector<int64_t> h_col_cnt;
  std::vector<int> h_upd_ptr, h_upd_lead;
  DevBuf<int2> upd_ij;
  // every layout: the (i, j) of the n_own_tiles tiles this workspace stores, in storage order (dense_ldl_list_tiles; the column
  // scaling and the masking of the shared-intrinsics border walk it)
  DevBuf<int2> own_tiles;
  int64_t n_own_tiles = 0;
  HipEvent ev_dtop, ev_dchain;  // distributed factorisation: fork behind the reduce of S, end of the owner's panel chain
};
typedef DenseLDLT<double> DenseLDL;
// the hoisted-diagonal schedule of dense_ldl_factor runs for HOIST_MIN_TILES + 2 <= nt <= HOIST_MAX_TILES
constexpr int HOIST_MIN_TILES = 32;  // below ~2 rounds of tiles the update is shorter than wait + factor
// The waiting workgroup keeps one CU of one XCD from the update, whose blocks the hardware deals round-robin to the
// XCDs: that XCD runs 32/31 longer and the launch ends with it -- 3 % of the update time, which grows as nt^3 while
// the hoisted 59 us per pair grow as nt.  Measured: n = 16002 (nt 126) 37.1 -> 35.6 ms, n = 40000 (nt 313) 411 -> 418 ms;
// the model's break-even is nt ~ 250.  (Since then the update's workgroups draw tickets, ticket_tile above, and the other XCDs
// empty that XCD's queue: at nt = 126 a launch takes 616 us in order, 652-655 beside the hoisted workgroup, 644-651 with
// tickets -- most of the loss is not that XCD's share)
constexpr int HOIST_MAX_TILES = 224;

// transport of the cross-rank sums (ba_comm.hip): RCCL called directly, or a caller-supplied hook
struct BaComm {
  int rank = 0, world = 1;
  ba_comm_fn hook = nullptr;
  void *hook_ctx = nullptr;
  void *nccl = nullptr;  // ncclComm_t
  int64_t calls = 0, bytes = 0;
  int64_t op_calls[BA_COMM_OPS] = {}, op_bytes[BA_COMM_OPS] = {};
  bool active() const { return hook != nullptr || nccl != nullptr; }  // a 1-rank communicator still exercises the path
};

void lm_free(ba_problem *p);  // the LM workspace (ba_lm.hip)

// one kind of Gaussian prior of a handle (ba_lm_set_priors): the host lists as given (indices 0-based), their device copies
struct PriorSet {
  int64_t n = 0;
  std::vector<int> h_idx;
  std::vector<double> h_mu, h_info;
  DevBuf<int> idx;
  DevBuf<double> mu, info;
};
enum { PRI_PNT = 0, PRI_CAM, PRI_CTR, PRI_KINDS };

// ---- block refinement (ba_refine_points, ba_refine_cameras, ba_resect_cameras, ba_ransac_cameras, ba_ransac_points) ------------------------------------------------
// One side of x is held and every block of the other side -- a point, a camera -- is its own small Marquardt problem.  What a
// call keeps whichever side it refines, and what the shared host code (block_* below) works on: the host entry's status /
// cost staging and the eight device counters
constexpr int BLOCK_COUNTERS = BA_PT_STATES + 2;  // [states | blocks flagged BEHIND | most trials of a block]
struct BlockWork {
  DevBuf<unsigned long long> counts;
  DevBuf<uint8_t> status;
  DevBuf<double> cost;
};

// points with the cameras held (ba_point_kernels.hip): the point list split by degree once per problem (wave_pts: degree > the
// tier threshold, one wave each; lane_pts: the others, one lane each, by descending degree) and the per-point lookup of the
// point priors (block_prior_lookup; rebuilt when ba_lm_set_priors changed them).
// ba_ransac_points (allocated at its first call): per observation the inlier byte and the masked copy of the information
// factors, per point the size of its set and the winning hypothesis -- nothing per hypothesis
struct PointWork : BlockWork {
  bool split = false;
  int64_t n_lane = 0, n_wave = 0;
  DevBuf<int> lane_pts, wave_pts;
  DevBuf<int> pri_of;
  int64_t pri_version = -1;
  DevBuf<uint8_t> rs_inlier;
  DevBuf<double> rs_info;
  DevBuf<int> rs_n, rs_best;
};

// cameras with the points held (ba_camera_kernels.hip): the per-camera lookups of the camera and of the centre priors (rebuilt
// when ba_lm_set_priors changed them), the effective 9-bit mask of held components -- the mask of ba_lm_set_fixed with the bits
// of (k1, k2, f) set for every member of a calibration group (rebuilt when ba_lm_set_fixed or ba_lm_set_shared_intrinsics
// changed them) -- and the byte per camera that k_resect_cameras leaves for k_refine_cameras (ba_resect_cameras).
// ba_ransac_cameras (allocated at its first call): per (camera, hypothesis) the pose and the inlier count, per observation the
// inlier byte and the masked copy of the information factors, per camera the size of its set, the winning hypothesis and the
// "stopped" byte of the refits, and the scratch copy of the cameras the refits resect into
struct CameraWork : BlockWork {
  DevBuf<int> cam_pri_of, ctr_pri_of;
  DevBuf<uint16_t> mask;
  bool mask_on = false;
  int64_t pri_version = -1, fix_version = -1, grp_version = -1;
  DevBuf<uint8_t> resect;
  DevBuf<double> hyp_pose, rs_info, rs_cams;
  DevBuf<int> hyp_count, rs_n, rs_best;
  DevBuf<uint8_t> rs_inlier, rs_stopped;
  int64_t hyp_cap = 0;  // hypotheses per camera that hyp_pose and hyp_count hold
  // ba_p3p: the triples (n x 3 x 2 image points, n x 3 x 3 world points), their poses (n x 4 x 6) and counts
  DevBuf<double> p3_q, p3_X, p3_pose;
  DevBuf<int> p3_n;
  int64_t p3_cap = 0;
};

// what the consensus kernels of ba_ransac_cameras work on (ba_ransac_kernels.hip; launched from ba_camera_kernels.hip)
struct RansacArgs {
  const int *cam_ptr, *cam_obs, *pnt0;
  const double *pt2d, *info;  // info: the caller's l00 l10 l11 per observation, or null
  const uint16_t *mask;       // effective mask of held components per camera, or null
  const double *x, *xc;       // the whole vector (the points are read from it) and its camera part (the intrinsics)
  double *hyp_pose;           // RANSAC_HYP_DOUBLES per (camera, hypothesis): r, t and the f it scores under
  int *hyp_count;             // inliers per (camera, hypothesis), -1: void
  uint8_t *inlier, *stopped;
  int *n_inliers, *best_hyp;
  int hypotheses, sample, min_inliers;
  uint64_t seed_mix;          // mix(seed)
  double tau2;
  int focal;                  // a camera whose f is free estimates it per hypothesis (ba_ransac_cameras_focal)
};
constexpr int RANSAC_HYP_DOUBLES = 7;
uint64_t ransac_seed_mix(uint64_t seed);  // mix(seed) of the header's sampling
// what solves a hypothesis: the linear resection of the sample (ba_ransac_cameras, _focal) or P3P (ba_ransac_cameras_p3p)
enum RansacGen { GEN_LINEAR = 0, GEN_P3P };
int launch_ransac_hypotheses(const RansacArgs &a, int64_t ncams, RansacGen gen, hipStream_t st);
int launch_ransac_select(const RansacArgs &a, int64_t ncams, hipStream_t st);
// the whole list of every camera that has not stopped under the pose of `cams` (9 per camera); resect: the byte
// k_resect_cameras left (2: no pose was found)
int launch_ransac_rescore(const RansacArgs &a, int64_t ncams, const double *cams, const uint8_t *resect, hipStream_t st);
// out (3 per observation) <- the caller's factors, or (1, 0, 1) when none is set, on the inliers; 0 elsewhere
int launch_ransac_mask_info(const RansacArgs &a, int64_t nobs, double *out, hipStream_t st);

// splitmix64: the one generator of the sampling (ba_ransac_sample), host and device
__host__ __device__ inline uint64_t ransac_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// list position of draw j of the hypothesis with key `key` in a list of d entries, d < 2^31
__host__ __device__ inline int64_t ransac_draw(uint64_t key, int j, int64_t d) {
  return (int64_t)(((ransac_mix(key ^ (uint64_t)j) >> 32) * (uint64_t)d) >> 32);
}
constexpr int RN_DRAWS = 64;  // draws per hypothesis: one per lane
constexpr int RS_P3P_SAMPLE = 3;  // the sample of a P3P hypothesis (ba_ransac_cameras_p3p)
// the limits of ba_ransac_opts: the largest sample, hypotheses per list (the selection key holds h in 12 bits) and refits
constexpr int RN_SAMPLE_MAX = 16, RN_HYP_MAX = 4096, RN_REFITS_MAX = 8;
// The options as the kernels take them (defaults filled in), or BA_ERR_ARG with `who` in the message.  least: the smallest
// sample and set of the caller's fit (RS_MIN_OBS of the resection, EP_MIN_MATCHES of the relative pose).  Where the sample of
// a hypothesis and the fit of a set differ (the five-point entry: a sample of exactly 5, sets of 8 for the eight-point fits
// behind it) least_set is the smallest set and most the largest sample; 0: least and RN_SAMPLE_MAX.
int ransac_opts_check(const char *who, const ba_ransac_opts *in, ba_ransac_opts *out, int least, int least_set = 0, int most = 0);

// ---- relative pose of camera pairs (ba_relative_pose; ba_pair_kernels.hip) -------------------------------------
// The per-call device buffers (allocated at the first call, grown when a call needs more): per pair the first match of its
// list, the six intrinsics (k1, k2, f of a, then of b), state, pose, set size, winner and "stopped" byte; per match its two
// observations, its pair, the ray record (q_a, q_b, used: PAIR_RAY doubles) and the inlier byte; per (pair, hypothesis) the
// pose (r, t) and the inlier count
constexpr int PAIR_RAY = 5, PAIR_HYP_DOUBLES = 6;
struct PairWork {
  DevBuf<int> match_ptr, obs_a, obs_b, pair_of, hyp_count, n_inliers, best_hyp;
  DevBuf<double> intr, rays, hyp_pose, pose;
  DevBuf<uint8_t> inlier, stopped, status;
  int64_t pair_cap = 0, match_cap = 0, hyp_cap = 0;
  // ba_five_point: the tuples (n x 5 x 2 per image), their solutions (n x 10 x 9) and counts
  DevBuf<double> five_qa, five_qb, five_E;
  DevBuf<int> five_n;
  int64_t five_cap = 0;
  // ba_refine_relative_pose: per pair the state, the two cost entries, |M'| under the returned pose and the trials
  DevBuf<uint8_t> rr_state;
  DevBuf<double> rr_cost;
  DevBuf<int> rr_consistent, rr_iters;
  int64_t rr_cap = 0;
  // ba_homography: H per (pair, hypothesis) and per pair (9 doubles each)
  DevBuf<double> hg_hyp, hg_H;
  int64_t hg_hyp_cap = 0, hg_cap = 0;
  // ba_homography_pose: per pair the parallax, the number of poses, two poses (r, unit t), their normals and supports
  DevBuf<double> hp_parallax, hp_pose, hp_normal;
  DevBuf<int> hp_n, hp_support;
  int64_t hp_cap = 0;
  // ba_decompose_homography: the matrices (n x 9), their solutions (n x 4 x 9, n x 4 x 3, n x 4 x 3), counts and parallaxes
  DevBuf<double> hd_H, hd_R, hd_t, hd_normal, hd_parallax;
  DevBuf<int> hd_n;
  int64_t hd_cap = 0;
};
// what the kernels of ba_relative_pose work on
struct PairArgs {
  const int *match_ptr, *obs_a, *obs_b, *pair_of;
  const double *intr, *pt2d, *info;  // info: the caller's l00 l10 l11 per observation, or null
  double *rays, *hyp_pose, *pose;
  int *hyp_count, *n_inliers, *best_hyp;
  uint8_t *inlier, *stopped, *status;
  int hypotheses, sample, min_inliers;  // hypotheses == 0: no consensus stage, the set is the used matches
  uint64_t seed_mix;                    // mix(seed)
  double tau2;
};
// what the kernels of ba_homography and ba_homography_pose take beside them (PairArgs keeps its layout: the kernels of
// ba_relative_pose keep their kernel arguments)
struct HomArgs {
  double *hyp_H, *H;  // 9 per (pair, hypothesis); 9 per pair
  // ba_homography_pose
  double *parallax, *pose2, *normal2;
  int *n_pose, *support2;
};
constexpr int HG_MIN_MATCHES = 4;          // 8 unknowns, two independent equations per match: the least sample and the least set
constexpr int HG_MIN_INLIERS_DEFAULT = 8;  // min_inliers <= 0
constexpr int HG_DOUBLES = 9;              // H per hypothesis and per pair, row-major
// the launches of ba_homography_kernels.hip (the entries are in ba_pair_kernels.hip, with the match lists and k_pair_rays)
int launch_hom_hypotheses(const PairArgs &a, const HomArgs &q, int64_t npairs, hipStream_t st);
int launch_hom_select(const PairArgs &a, const HomArgs &q, int64_t npairs, hipStream_t st);
int launch_hom_fit(const PairArgs &a, const HomArgs &q, int64_t npairs, int final, hipStream_t st);
int launch_hom_pose(const PairArgs &a, const HomArgs &q, int64_t npairs, hipStream_t st);
int launch_hom_decompose(int64_t n, const double *H, double *R, double *t, double *normal, int *n_sol, double *parallax, hipStream_t st);
// what k_pair_refine takes beside them (ba_refine_relative_pose; the options with their defaults filled in)
struct PairRefineArgs {
  uint8_t *state;
  double *cost;
  int *n_consistent, *iters;
  int max_iter, loss, all_used;  // all_used: the caller gave no set, it is every used match
  double xtol, lambda0, c2;
};
// the limits of ba_pair_refine_opts
constexpr int RR_MAX_ITER_DEFAULT = 50, RR_ROUNDS_DEFAULT = 2, RR_ROUNDS_MAX = 8;
constexpr double RR_XTOL_DEFAULT = 1e-10, RR_LAMBDA0_DEFAULT = 1e-4;
// The options as k_pair_refine takes them (defaults filled in), or BA_ERR_ARG with `who` in the message
int pair_refine_opts_check(const char *who, const ba_pair_refine_opts *in, ba_pair_refine_opts *out);

// ---- rotation averaging over the view graph (ba_rotation_loops, ba_average_rotations; ba_rotavg_kernels.hip) ---------
// The per-call device buffers, each grown when a call needs more.  Per pair: its cameras
// (0-based), the rotation vector and the 3 x 3 of it, the flags used / kept / "r is finite", the weight, the loop counts, the
// residual, rho' and the cost term.  Per camera: the CSR adjacency (ptr; nbr and edge per entry), the two buffers of the
// simultaneous update, the start (the gauge returns to it), held or not, the component, the root whose gauge is restored, the
// returned rotation vector.  cost: before, after.  delta: one slot per sweep.
// a device buffer that is grown when a call needs more (cap: the elements it holds)
template <typename T>
struct GrowBuf {
  DevBuf<T> d;
  int64_t cap = 0;
  operator T *() const { return d; }
};
struct RotavgWork {
  GrowBuf<int> pa, pb, adj_ptr, adj_nbr, adj_edge, n_loops, support, comp, root;
  GrowBuf<uint8_t> used, kept, finite, fixed;
  GrowBuf<double> r_rel, Rrel, weight, residual, edge_weight, term, R[2], Rstart, r, cost, delta;
};

// b <- at least n elements
template <typename T>
inline int grow(GrowBuf<T> &b, int64_t n) {
  if (b.cap >= n && b.d) return BA_OK;
  b.cap = 0;
  BA_CHECK(b.d.alloc(n));
  b.cap = n > 0 ? n : 1;
  return BA_OK;
}

// b <- the host vector h
template <typename T>
inline int put(GrowBuf<T> &b, const std::vector<T> &h, hipStream_t st) {
  BA_CHECK(grow(b, (int64_t)h.size()));
  if (!h.empty()) BA_HIP_CHECK(hipMemcpyAsync((T *)b, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return BA_OK;
}

// ---- translation averaging over the view graph (ba_translation_loops, ba_average_translations; ba_transavg_kernels.hip)
// The per-call device buffers.  Per pair: its cameras (0-based), the direction as given and normalised, the flags used / kept /
// "the direction is usable", the weight, the loop counts, the two linearisations (current and trial: A 6, g 3, the cost term),
// the residual and rho'.  Per camera: the CSR adjacency, the two positions (current, trial), held or not, the component, the
// gathered gradient, lambda diag H, the preconditioner (6), "takes part in the solve", and the vectors of the conjugate
// gradient (x, r, z, p, q: 3 each) with the per-camera terms of its dot products.  sc: the scalars of a solve (rz, |r0|_M,
// alpha, the bound |r|_M has to reach); st: done, iterations; cost: before, after, trial.
struct TransavgWork {
  GrowBuf<int> pa, pb, adj_ptr, adj_nbr, adj_edge, n_loops, support, comp, st;
  GrowBuf<uint8_t> used, kept, finite, fixed, active;
  GrowBuf<double> dir_in, dir, weight, A[2], g[2], term[2], residual, edge_weight, c[2], gc, dg, Minv, x, r, z, p, q, part, sc, cost;
};

// ---- similarity alignment of reconstructions (ba_similarity; ba_similarity_kernels.hip) ------------------------------
// The per-call device buffers.  Per problem: the first row of its list, state, set size, winner, "stopped" byte, the returned
// (s, r, t) and rms; per row its record (src, dst, used: 7 doubles, packed on the host) and the inlier byte; per (problem,
// hypothesis) the fit (s, R, t: 13 doubles) and the inlier count
struct SimilarityWork {
  GrowBuf<int> row_ptr, hyp_count, n_inliers, best_hyp;
  GrowBuf<double> rows, hyp, sim, rms;
  GrowBuf<uint8_t> inlier, stopped, status;
};
// what the kernels of ba_similarity work on
struct SimArgs {
  const int *row_ptr;
  const double *rows;
  double *hyp, *sim, *rms;
  int *hyp_count, *n_inliers, *best_hyp;
  uint8_t *inlier, *stopped, *status;
  int hypotheses, sample, min_inliers, with_scale;  // hypotheses == 0: no consensus stage, the set is the used rows
  uint64_t seed_mix;                                // mix(seed)
  double tau2;
};
constexpr int SM_MIN_ROWS = 3;  // three rows that are not collinear fix a similarity: the least sample and the least set

struct ba_problem {
  int device = 0;
  HipStream stream;
  int64_t ncams = 0, npnts = 0, nobs = 0;
  // device mirrors (0-based int32)
  DevBuf<int> cam0, pnt0;
  DevBuf<double> pt2d;
  DevBuf<float> pt2d_f32;
  // observation lists sorted by point / by camera (stable) for the deterministic reductions
  DevBuf<int> pt_ptr, pt_obs;    // npnts+1, nobs
  DevBuf<int> cam_ptr, cam_obs;  // ncams+1, nobs
  bool point_sorted = false;                   // observations already grouped by point (BAL order)
  std::vector<int> h_cam0, h_pnt0, h_pt_ptr, h_pt_obs;
  // scratch for the host-pointer entries
  DevBuf<char> scratch[4];
  size_t scratch_bytes[4] = {0, 0, 0, 0};
  // LM workspace (allocated at the first solve, ba_lm.hip; released by lm_free)
  struct LMWork *lm = nullptr;
  // robust loss of the LM entries (ba_lm_set_loss): BA_LOSS_*, scale c > 0
  int loss = BA_LOSS_LINEAR;
  double loss_scale = 1.0;
  // fixed parameters of the LM entries (ba_lm_set_fixed): host masks (empty: none of that kind), counts, and their device
  // copies (allocated at the first upload, ncams / npnts entries: never reallocated), uploaded lazily (fix_dirty)
  std::vector<uint16_t> h_fix_cam;
  std::vector<uint8_t> h_fix_pnt;
  int64_t fix_ncam = 0, fix_npnt = 0;  // fixed camera components, fixed points
  DevBuf<uint16_t> d_fix_cam;
  DevBuf<uint8_t> d_fix_pnt;
  bool fix_dirty = false;
  int64_t fix_version = 0;  // counts the calls of ba_lm_set_fixed (CameraWork keeps a table derived from the camera masks)
  bool fix_on() const { return fix_ncam > 0 || fix_npnt > 0; }
  // Gaussian priors of the LM entries (ba_lm_set_priors): points, cameras, camera centres; uploaded lazily (pri_dirty, prior_upload)
  // with the buffers the prior kernels write: pri_d = d_k = h_k(x) - mu_k at the linearisation (3 / 9 / 3 per prior, kind after
  // kind), pri_H = H_k of the centre priors (3 x 6 each, columns of fixed components zeroed), pri_val = three arrays of one value
  // per prior (kind after kind): d'Lambda d at the linearisation, at the trial point, and the step's model term
  PriorSet pri[PRI_KINDS];
  bool pri_dirty = false;
  int64_t pri_version = 0;  // counts the calls of ba_lm_set_priors (PointWork and CameraWork keep tables derived from the priors)
  DevBuf<double> pri_d, pri_H, pri_val;
  int64_t pri_total() const { return pri[PRI_PNT].n + pri[PRI_CAM].n + pri[PRI_CTR].n; }
  bool pri_on() const { return pri_total() > 0; }
  double *pri_cost() const { return pri_val; }
  double *pri_cost_trial() const { return pri_val + pri_total(); }
  double *pri_model() const { return pri_val + 2 * pri_total(); }
  // shared intrinsics of the LM entries (ba_lm_set_shared_intrinsics): the labels as kept (0 = own; groups with one member
  // dropped, the others renumbered 1..grp_n in the order of their labels), the members of every group in ascending camera
  // order (h_grp_mem[h_grp_ptr[g] .. h_grp_ptr[g + 1]), 0-based cameras; the first is the member that carries the group's
  // entries of the z vector), and their device copies in camera order (uploaded lazily, shared_upload): grp_ptr, grp_row =
  // 9 camera + 6 of every member.  grp_version counts the changes (the LM workspace keeps tables in the order of S).
  std::vector<int> h_grp, h_grp_ptr, h_grp_mem;
  int grp_n = 0;
  int64_t grp_version = 0;
  bool grp_dirty = false;
  DevBuf<int> grp_ptr, grp_row;
  bool grp_on() const { return grp_n > 0; }
  // per-observation information of the LM entries (ba_lm_set_obs_info): the factors L_i of Lambda_i = L_i L_i' (l00 l10 l11 per
  // observation, caller's order; empty: none), how many Lambda_i are all zero, a count of the arrays set so far (a recorded
  // sequence is keyed on it), and the device copy (allocated at the first upload, 3 nobs entries: never reallocated),
  // uploaded lazily (info_dirty, info_upload)
  std::vector<double> h_info;
  bool info_set = false, info_dirty = false;
  int64_t info_zero = 0, info_version = 0;
  DevBuf<double> d_info;
  bool info_on() const { return info_set; }
  PointWork pts;
  CameraWork cams;
  PairWork pairs;
  RotavgWork rotavg;
  TransavgWork transavg;
  SimilarityWork similarity;
  // communication (multi-GPU)
  int rank = 0, world = 1;
  BaComm comm;
  // profiling
  bool prof_on = false;
  ProfSlot prof[PC_COUNT];
  HipEvent ev0, ev1;
  ~ba_problem() { lm_free(this); }
};

// RAII-less helper: times one kernel class with an event pair when profiling is on (synchronises).
struct ProfScope {
  ba_problem *p;
  int cls;
  hipStream_t st;
  ProfScope(ba_problem *p_, int cls_, hipStream_t st_) : p(p_), cls(cls_), st(st_) {
    if (p->prof_on) (void)hipEventRecord(p->ev0, st);
  }
  ~ProfScope() {
    if (p->prof_on) {
      (void)hipEventRecord(p->ev1, st);
      (void)hipEventSynchronize(p->ev1);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, p->ev0, p->ev1);
      p->prof[cls].ms += ms;
      p->prof[cls].calls += 1;
    }
  }
};

int ba_scratch(ba_problem *p, int slot, size_t bytes, void **out);

// ---- host side of the block refinements (ba_api.hip; the two with a callable here) ----------------------------------------
// out <- the table "block -> its prior of `set`, or -1" over nblocks blocks; nothing for an empty set
int block_prior_lookup(const PriorSet &set, int64_t nblocks, DevBuf<int> &out);
// the device counters of w -> the caller's (either may be null; synchronises st)
int block_counts(const BlockWork &w, int64_t *counts, int *iters_max, hipStream_t st);

// The argument tests of an entry, `who` in their messages: null arguments, then own() -- the entry's own refusal, BA_OK or an
// error it has set --, then finite tolerances; values below their range become the defaults.
template <typename Own>
int block_check(const char *who, ba_problem *p, const double *x, int max_iter_default, int *max_iter, double *xtol, double *lambda0, Own own) {
  if (!p || (!x && p->npnts + p->ncams > 0)) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  BA_CHECK(own());
  if (!std::isfinite(*xtol) || !std::isfinite(*lambda0)) {
    ba_set_error("%s: xtol and lambda0 must be finite (<= 0: the default), got %g and %g", who, *xtol, *lambda0);
    return BA_ERR_ARG;
  }
  if (*max_iter < 0) *max_iter = max_iter_default;
  if (*xtol <= 0) *xtol = 1e-10;
  if (*lambda0 <= 0) *lambda0 = 1e-4;
  return BA_OK;
}

// The body of a host-pointer entry: x into scratch, launch(d_x, d_status, d_cost, st), back the refined part of x (n blocks of
// `per` doubles from `offset` on: the rest of the caller's x is never written) with its status and cost, then the counters.
template <typename Launch>
int block_host_entry(ba_problem *p, BlockWork &w, double *x_inout, int64_t n, int per, int64_t offset, uint8_t *status, double *cost,
                     int64_t *counts, int *iters_max, Launch launch) {
  BA_HIP_CHECK(hipSetDevice(p->device));
  const int64_t nvar = 9 * p->ncams + 3 * p->npnts;
  hipStream_t st = p->stream;
  double *dx;
  BA_CHECK(ba_scratch(p, 0, (size_t)(nvar + 1) * sizeof(double), (void **)&dx));
  if (status && !w.status) BA_CHECK(w.status.alloc(n));
  if (cost && !w.cost) BA_CHECK(w.cost.alloc(2 * n));
  BA_HIP_CHECK(hipMemcpyAsync(dx, x_inout, (size_t)nvar * sizeof(double), hipMemcpyHostToDevice, st));
  BA_CHECK(launch(dx, status ? (uint8_t *)w.status : nullptr, cost ? (double *)w.cost : nullptr, st));
  if (n > 0) {
    BA_HIP_CHECK(hipMemcpyAsync(x_inout + offset, dx + offset, (size_t)per * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status) BA_HIP_CHECK(hipMemcpyAsync(status, w.status, (size_t)n, hipMemcpyDeviceToHost, st));
    if (cost) BA_HIP_CHECK(hipMemcpyAsync(cost, w.cost, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BA_HIP_CHECK(hipStreamSynchronize(st));
  return block_counts(w, counts, iters_max, st);
}

// ---- launchers (ba_model_kernels.hip) -----------------------------------------------------------
int launch_residual_f64(ba_problem *p, const double *d_x, double *d_r, hipStream_t st);
int launch_residual_f32(ba_problem *p, const float *d_x, float *d_r, hipStream_t st);
int launch_jac_structure(ba_problem *p, int64_t *d_rows, int64_t *d_cols, hipStream_t st);
int launch_jac_coord_f64(ba_problem *p, const double *d_x, double *d_vals, hipStream_t st);
int launch_jac_coord_f32(ba_problem *p, const float *d_x, float *d_vals, hipStream_t st);
// the cam_pre rows of the cameras of d_x (CPAD doubles per camera) in the scratch the residual and Jacobian launchers use
int launch_cam_pre_f64(ba_problem *p, const double *d_x, const double **d_cpre, hipStream_t st);

// ---- launchers (ba_normal_kernels.hip) ----------------------------------------------------------
// point side: H_pp (6/pt: xx,xy,xz,yy,yz,zz) and g_p (3/pt) from J, r.  Either output may be null.
int launch_point_blocks(ba_problem *p, const double *d_J, const double *d_r, double *d_Hpp, double *d_gp,
                        hipStream_t st);
// camera side: H_cc (45/cam packed lower row-major) and g_c (9/cam).  Either output may be null.
int launch_cam_blocks(ba_problem *p, const double *d_J, const double *d_r, double *d_Hcc, double *d_gc,
                      hipStream_t st);

// ---- dense LDL^T (ba_dense_ldl.hip) ---------------------------------------------------------------
template <typename T>
int dense_ldl_alloc(DenseLDLT<T> *w, int64_t n_unpadded, int world = 1, int rank = 0, bool lazy_S = false, bool own_only = false);
// lazy_S: the tiles of S (and the panel buffers V) are left out until dense_ldl_alloc_S
template <typename T>
int dense_ldl_alloc_S(DenseLDLT<T> *w);
int64_t dense_ldl_tiles_doubles(int64_t n_unpadded);  // number of ELEMENTS of the packed lower tiles
// factor S in place (L below the diagonal tiles' diagonal, D separately); an exactly zero pivot sets DenseLDLT::flag.
// d_b != null: the forward substitution L y = b of that right-hand side (length nt*NB, clobbered) is fused into the
// panel solves; pass forward_done = true to dense_ldl_solve afterwards.
template <typename T>
int dense_ldl_factor(ba_problem *p, DenseLDLT<T> *w, hipStream_t st, T *d_b);
// the same factorisation with the tile column pairs distributed over the ranks of p->comm (owner of pair q: q % world):
// on entry rank r holds the (summed) tile columns it owns, on exit every rank holds the complete factor (L, Linv, D).
// No fused forward substitution: call dense_ldl_solve(..., forward_done = false).
template <typename T>
int dense_ldl_factor_dist(ba_problem *p, DenseLDLT<T> *w, hipStream_t st, T *d_b = nullptr);
// block-sparse S: the use of a tile pattern (tile_pattern_build, ba_order.h) by a workspace (null: dense).  The pattern object
// must outlive the workspace.
template <typename T>
int dense_ldl_use_pattern(DenseLDLT<T> *w, const TilePattern *pat);
// DenseLDLT::own_tiles of the workspace's current layout (after dense_ldl_use_pattern, where a pattern is used)
int dense_ldl_list_tiles(DenseLDLT<double> *w);
// solve S x = b for one right-hand side held in d_b (length nt*NB, overwritten by x)
template <typename T>
int dense_ldl_solve(ba_problem *p, DenseLDLT<T> *w, T *d_b, hipStream_t st, bool forward_done);

// the factor applied to m right-hand sides at once (one GPU, dense or block-sparse S): column c of d_B (ld = its stride, >= nt NB)
// is overwritten by S^-1 of it; d_y: m * ld elements of scratch.  Forward and backward sweeps, nt launches each.
template <typename T>
int dense_ldl_solve_multi(ba_problem *p, DenseLDLT<T> *w, T *d_B, int64_t ld, int m, T *d_y, hipStream_t st);

// ---- transport (ba_comm.hip): all on stream st, in place, no-ops without a communicator --------------------
int comm_allreduce(ba_problem *p, double *d_buf, int64_t count, hipStream_t st);
int comm_reduce(ba_problem *p, double *d_buf, int64_t count, int root, hipStream_t st);  // sum lands on root only
int comm_reduce_f32(ba_problem *p, float *d_buf, int64_t count, int root, hipStream_t st);
int comm_bcast(ba_problem *p, void *d_buf, int64_t bytes, int root, hipStream_t st);
// d_buf: world segments of `count` elements (Float64, or Float32 when f32); segment `rank` receives the sum, in place
int comm_reduce_scatter(ba_problem *p, void *d_buf, int64_t count, bool f32, hipStream_t st);
int comm_group_begin(ba_problem *p);  // RCCL: fuse the calls up to comm_group_end into one launch
int comm_group_end(ba_problem *p);
void comm_free(ba_problem *p);
