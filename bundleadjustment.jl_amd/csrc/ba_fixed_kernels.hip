// Fixed parameters of the LM solve (ba_lm_set_fixed, include/ba_hip.h): the masking pass k_fix_mask and the entries that set
// and read the mask of a handle.
//
// The LM loop minimises over the free entries of x only.  k_fix_mask zeroes the columns of the fixed parameters in the
// stored Jacobian J right after it is evaluated; everything downstream (the point and camera blocks, the Schur assembly, the
// factorisations, PCG, the model value, the sharded path) then runs unchanged: the fixed entries of J'r are exactly 0, their
// rows and columns of J'J hold only the damping, so their step is exactly 0 and the free part of the step is that of the
// problem restricted to the free variables.
#include "ba_internal.h"
#include "ba_lm_internal.h"

namespace {

constexpr int FB = OBS_TILE;  // observations per workgroup = threads per workgroup

// One workgroup = FB consecutive observations.  Thread t builds the 12-bit mask of fixed Jacobian columns of observation t
// (bits 0..2 the point, bits 3..11 the camera components: column c of J is bit c) from the int32 camera / point index and the
// small per-camera / per-point tables, and puts it in LDS.  A workgroup none of whose observations has a fixed column ends
// there.  Otherwise the tile's 12 FB 16-byte vectors of J are visited by the whole workgroup, vector k FB + t by thread t
// (contiguous across the lanes of a wave, as k_obs_scale streams them): vector e of an observation holds columns 2 (e % 6)
// and 2 (e % 6) + 1 of row e / 6.  Only zeros are stored, and only where a column is fixed: 16 bytes when both columns of
// the vector are fixed, 8 bytes when one is.  J itself is never read.  CAM / PNT: whether the camera / point table is
// present (the indices of a kind without a table are not read).
template <bool CAM, bool PNT>
__global__ __launch_bounds__(FB) void k_fix_mask(int64_t nobs, const int *__restrict__ cam0, const int *__restrict__ pnt0,
                                                 const uint16_t *__restrict__ cam_mask, const uint8_t *__restrict__ pnt_fixed,
                                                 double2 *__restrict__ J) {
  __shared__ uint16_t sm[FB];
  const int t = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * FB, o = o0 + t;
  unsigned m = 0;
  if (o < nobs) {
    if (CAM) m = (unsigned)cam_mask[cam0[o]] << 3;
    if (PNT && pnt_fixed[pnt0[o]]) m |= 7u;
  }
  sm[t] = (uint16_t)m;
  if (!__syncthreads_or(m != 0)) return;  // (uniform across the workgroup)
  const int nv = (int)((nobs - o0 < FB ? nobs - o0 : FB) * JV);  // vectors of this tile
  double2 *__restrict__ Jt = J + o0 * JV;
  double *__restrict__ Jd = reinterpret_cast<double *>(Jt);
#pragma unroll
  for (int k = 0; k < JV; k++) {
    const int v = k * FB + t;
    if (v < nv) {
      const int e = v % JV;
      const unsigned bits = ((unsigned)sm[v / JV] >> (2 * (e % 6))) & 3u;
      if (bits == 3u) Jt[v] = make_double2(0.0, 0.0);
      else if (bits == 1u) Jd[2 * v] = 0.0;
      else if (bits == 2u) Jd[2 * v + 1] = 0.0;
    }
  }
}

}  // namespace

// the handle's mask to the device, once per change (ba_lm_set_fixed marks it dirty).  The tables are allocated at their
// full size at the first upload and never reallocated; a handle whose mask is cleared keeps them (unused).
int fix_upload(ba_problem *p) {
  if (!p->fix_dirty) return BA_OK;
  if (p->fix_ncam > 0) {
    if (!p->d_fix_cam) BA_CHECK(p->d_fix_cam.alloc(p->ncams));
    BA_HIP_CHECK(hipMemcpyAsync(p->d_fix_cam, p->h_fix_cam.data(), (size_t)p->ncams * sizeof(uint16_t), hipMemcpyHostToDevice,
                                p->stream));
  }
  if (p->fix_npnt > 0) {
    if (!p->d_fix_pnt) BA_CHECK(p->d_fix_pnt.alloc(p->npnts));
    BA_HIP_CHECK(hipMemcpyAsync(p->d_fix_pnt, p->h_fix_pnt.data(), (size_t)p->npnts, hipMemcpyHostToDevice, p->stream));
  }
  BA_HIP_CHECK(hipStreamSynchronize(p->stream));  // (the host tables may change with the next ba_lm_set_fixed)
  p->fix_dirty = false;
  return BA_OK;
}

int launch_fix_mask(ba_problem *p, double *d_J, hipStream_t st) {
  if (!p->fix_on() || p->nobs <= 0) return BA_OK;
  ProfScope ps(p, PC_FIXED, st);
  const unsigned nb = grid_for(p->nobs, FB);
  const bool cam = p->fix_ncam > 0, pnt = p->fix_npnt > 0;
  if (cam && pnt)
    return BA_LAUNCH((k_fix_mask<true, true>), nb, FB, 0, st, p->nobs, p->cam0, p->pnt0, p->d_fix_cam, p->d_fix_pnt, (double2 *)d_J);
  if (cam) return BA_LAUNCH((k_fix_mask<true, false>), nb, FB, 0, st, p->nobs, p->cam0, p->pnt0, p->d_fix_cam, nullptr, (double2 *)d_J);
  return BA_LAUNCH((k_fix_mask<false, true>), nb, FB, 0, st, p->nobs, p->cam0, p->pnt0, nullptr, p->d_fix_pnt, (double2 *)d_J);
}

extern "C" int ba_lm_set_fixed(ba_problem *p, const uint16_t *cam_mask, const uint8_t *pnt_fixed) {
  if (!p) {
    ba_set_error("ba_lm_set_fixed: null handle");
    return BA_ERR_ARG;
  }
  int64_t ncam = 0, npnt = 0;
  if (cam_mask)
    for (int64_t c = 0; c < p->ncams; c++) {
      if (cam_mask[c] > 0x1FF) {
        ba_set_error("ba_lm_set_fixed: cam_mask[%lld] = 0x%x has a bit above 8 (a camera has 9 components)", (long long)c,
                     (unsigned)cam_mask[c]);
        return BA_ERR_ARG;
      }
      ncam += __builtin_popcount(cam_mask[c]);
    }
  if (pnt_fixed)
    for (int64_t j = 0; j < p->npnts; j++) {
      if (pnt_fixed[j] > 1) {
        ba_set_error("ba_lm_set_fixed: pnt_fixed[%lld] = %u, must be 0 or 1", (long long)j, (unsigned)pnt_fixed[j]);
        return BA_ERR_ARG;
      }
      npnt += pnt_fixed[j];
    }
  // (no workspace is touched here: the mask may be set before or after the communicator, before the first solve)
  p->fix_ncam = ncam;
  p->fix_npnt = npnt;
  if (ncam > 0) p->h_fix_cam.assign(cam_mask, cam_mask + p->ncams);
  else p->h_fix_cam.clear();
  if (npnt > 0) p->h_fix_pnt.assign(pnt_fixed, pnt_fixed + p->npnts);
  else p->h_fix_pnt.clear();
  p->fix_dirty = p->fix_on();
  p->fix_version++;
  return BA_OK;
}

extern "C" int ba_lm_get_fixed(const ba_problem *p, int64_t *n_fixed_cam_params, int64_t *n_fixed_points) {
  if (!p) {
    ba_set_error("ba_lm_get_fixed: null handle");
    return BA_ERR_ARG;
  }
  if (n_fixed_cam_params) *n_fixed_cam_params = p->fix_ncam;
  if (n_fixed_points) *n_fixed_points = p->fix_npnt;
  return BA_OK;
}
