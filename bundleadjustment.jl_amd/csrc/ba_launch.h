// The one place a kernel of libba_hip.so is launched from (tests/test_host.py), and the grid arithmetic of the launch sites.
// Included by ba_internal.h (after BA_OK / BA_ERR_HIP and ba_set_error).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// workgroups of `block` work-items that cover n items
inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// kernel<<<grid, block, lds, st>>>(args...), reached through BA_LAUNCH.  Every parameter of the kernel is named at the site
// and converted to the parameter's type there (a plain nullptr, an int for an int64_t, a DevBuf<T> for a T *).  A grid with
// a zero dimension is no work: BA_OK, nothing launched.  A launch the runtime refuses sets the error message "<file>:<line>:
// <kernel as written at the site> -> <HIP's error string>" and returns BA_ERR_HIP.
template <typename... KArgs, typename... Args>
[[nodiscard]] int ba_launch(const char *name, const char *file, int line, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds,
                            hipStream_t st, Args &&...args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "a launch site names every parameter of its kernel");
  if (grid.x == 0 || grid.y == 0 || grid.z == 0) return BA_OK;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<KArgs>(args)...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ba_set_error("%s:%d: %s -> %s", file, line, name, hipGetErrorString(e));
    return BA_ERR_HIP;
  }
  return BA_OK;
}
// (a kernel whose template arguments contain a comma goes in parentheses)
#define BA_LAUNCH(kernel, grid, block, lds, st, ...) \
  ba_launch(#kernel, __FILE__, __LINE__, kernel, dim3(grid), dim3(block), lds, st, __VA_ARGS__)
