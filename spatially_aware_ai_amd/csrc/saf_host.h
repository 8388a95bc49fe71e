// saf_host.h -- host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/saf.h"
#include "saf_knobs.h"

namespace saf {

// Thread-local message behind saf_last_error(); defined in saf_fuse.hip.
char* err_buf();
constexpr size_t kErrLen = 512;

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), kErrLen, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SAF_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return SAF_OK;
}

inline int64_t n_voxels(const saf_volume* v) { return (int64_t)v->nx * v->ny * v->nz; }

inline int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
  return cus;
}

// Workgroups of a grid-stride launch: one per `per_wg` items, no more than `per_cu` for each compute unit, at least one.
inline unsigned grid_1d(int64_t items, int per_cu, int per_wg = 256) {
  int64_t blocks = (items + per_wg - 1) / per_wg;
  const int64_t cap = (int64_t)device_cus() * per_cu;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// Before a launch with `bytes` of dynamic LDS: above the 64 KB every kernel may ask for, the kernel's own limit is raised to them.
template <typename K>
inline int allow_lds(K* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return SAF_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return fail(SAF_E_HIP, "hipFuncSetAttribute(LDS=%zu): %s", bytes, hipGetErrorString(e));
  return SAF_OK;
}

// One template argument from a run-time element type: f(std::integral_constant<int, DT>{}), so that `decltype(dt)::value` names the
// instantiation.  dispatch_ft: a feature dtype the entry point has checked (anything else counts as SAF_F32); dispatch_ft16: one it
// has checked to be 16-bit; dispatch_dtype: an unchecked one -- for any other value the caller's refusal `bad()` is the result.
// (The order of the cases is the order in which a file's kernels are instantiated and so laid out in its code object: a launch
//  switch whose cases stand in another order -- clip_tiles, dwconv7x7 -- keeps its kernels' order only by staying a switch.)
template <typename F>
int dispatch_ft(int ft, F&& f) {
  switch (ft) {
    case SAF_BF16: return f(std::integral_constant<int, SAF_BF16>{});
    case SAF_F16: return f(std::integral_constant<int, SAF_F16>{});
    default: return f(std::integral_constant<int, SAF_F32>{});
  }
}
template <typename F>
int dispatch_ft16(int ft, F&& f) {
  return ft == SAF_BF16 ? f(std::integral_constant<int, SAF_BF16>{}) : f(std::integral_constant<int, SAF_F16>{});
}
template <typename F, typename Bad>
int dispatch_dtype(int dt, F&& f, Bad&& bad) {
  switch (dt) {
    case SAF_F32: return f(std::integral_constant<int, SAF_F32>{});
    case SAF_F16: return f(std::integral_constant<int, SAF_F16>{});
    case SAF_BF16: return f(std::integral_constant<int, SAF_BF16>{});
    default: return bad();
  }
}

// A volume that the field readers (saf_field_dev.h) can use: two voxels per axis for a cell, int32 voxel indices, and the tsdf,
// its weights and the axis tables.  `also` is whatever else the entry `what` needs of the volume.
inline int check_field_volume(const char* what, const saf_volume* vol, bool also = true) {
  if (vol->nx < 2 || vol->ny < 2 || vol->nz < 2 || n_voxels(vol) > 0x7fffffff || !vol->tsdf || !vol->tsdf_weight || !vol->axis_x ||
      !vol->axis_y || !vol->axis_z || !also)
    return fail(SAF_E_INVALID, "%s: bad volume (%d x %d x %d voxels; at least 2 per axis, fewer than 2^31 in all)", what, (int)vol->nx,
                (int)vol->ny, (int)vol->nz);
  return SAF_OK;
}

// int32 pixel indices
inline int check_pixel_count(const char* what, int height, int width) {
  if ((int64_t)height * width > 0x7fffffff) return fail(SAF_E_INVALID, "%s: too many pixels", what);
  return SAF_OK;
}

}  // namespace saf
