// saf_field_dev.h -- reading the fused TSDF as a field, shared by the ray cast (saf_raycast.hip) and the pose linearisation
// (saf_track.hip): the grid frame from the axis tables, a pixel's camera ray, the plain-pinhole test, and the trilinear sample
// over eight voxel centres with the intermediates of its blend.
//
// This is the one C statement of the numerics contract that include/saf.h gives for saf_raycast and saf_pose_linearize
// (tests/raycast_reference.py and tests/pose_reference.py restate it in NumPy): every fp32 operation below is written on its
// own, in the order stated there.  Translation units that include this are compiled with -ffp-contract=off; divisions are IEEE.
#pragma once
#include "saf_common.h"
#include "saf_host.h"

#pragma clang fp contract(off)

namespace saf {

// two values that are consecutive along z: one 8-byte request (4-byte aligned) instead of two
struct __attribute__((packed, aligned(4))) PairF {
  float a, b;
};
struct __attribute__((packed, aligned(4))) PairI {
  int a, b;
};

// What a kernel needs to read the field.  check_field_volume (saf_host.h) is what makes these safe to use.
struct FieldArgs {
  const float* tsdf;
  const int* tsdf_weight;
  const float* axis_x;
  const float* axis_y;
  const float* axis_z;
  int nx, ny, nz;
};

inline FieldArgs field_args(const saf_volume* vol) {
  FieldArgs f;
  f.tsdf = vol->tsdf;
  f.tsdf_weight = vol->tsdf_weight;
  f.axis_x = vol->axis_x;
  f.axis_y = vol->axis_y;
  f.axis_z = vol->axis_z;
  f.nx = vol->nx;
  f.ny = vol->ny;
  f.nz = vol->nz;
  return f;
}

// the grid: voxel centre i of an axis at axis[i]; voxel size from the x table's ends
struct GridFrame {
  float ox, oy, oz, vs;
};
__device__ __forceinline__ GridFrame grid_frame(const FieldArgs& F) {
  GridFrame g;
  g.ox = F.axis_x[0];
  g.oy = F.axis_y[0];
  g.oz = F.axis_z[0];
  g.vs = (F.axis_x[F.nx - 1] - g.ox) / (float)(F.nx - 1);
  return g;
}

// the camera ray of pixel (u, v) at z = 1
__device__ __forceinline__ void pixel_ray(const float* K, int u, int v, float& dcx, float& dcy) {
  dcx = ((float)u - K[2]) / K[0];
  dcy = ((float)v - K[5]) / K[4];
}

// Unsupported intrinsics (skew, a third row other than 0 0 1) cannot be refused on the host without reading device memory.
__device__ __forceinline__ bool is_pinhole(const float* K) {
  return K[1] == 0.0f && K[3] == 0.0f && K[6] == 0.0f && K[7] == 0.0f && K[8] == 1.0f;
}

// floor(g) clamped to [0, n - 2] (any g, NaN included, gives a cell inside the grid) and the offset from it
__device__ __forceinline__ int cell_of(float g, int n, float& frac) {
  int i = (int)__builtin_floorf(g);
  i = i < 0 ? 0 : i;
  i = i > n - 2 ? n - 2 : i;
  frac = g - (float)i;
  return i;
}

__device__ __forceinline__ float lerp(float a, float b, float f) {
  const float d = b - a;
  const float m = f * d;
  return a + m;
}

// One trilinear sample: the eight corners as z-pairs at (x, y), (x, y + 1), (x + 1, y), (x + 1, y + 1), the offsets within the
// cell, and the blend z then y then x with its intermediates (a gradient is formed from the same ones).
struct FieldSample {
  PairF t00, t01, t10, t11;
  float fx, fy, fz;
  float c00, c01, c10, c11;
  float c0, c1;
  float value;
  bool observed;  // all 8 corners have tsdf_weight > 0
};

__device__ __forceinline__ FieldSample sample_field(const FieldArgs& F, float gx, float gy, float gz) {
  FieldSample s;
  const int ix = cell_of(gx, F.nx, s.fx);
  const int iy = cell_of(gy, F.ny, s.fy);
  const int iz = cell_of(gz, F.nz, s.fz);
  const int p00 = (ix * F.ny + iy) * F.nz + iz;  // < nx ny nz < 2^31 (checked on the host)
  const int p01 = p00 + F.nz;
  const int p10 = p00 + F.ny * F.nz;
  const int p11 = p10 + F.nz;
  s.t00 = *reinterpret_cast<const PairF*>(F.tsdf + p00);
  s.t01 = *reinterpret_cast<const PairF*>(F.tsdf + p01);
  s.t10 = *reinterpret_cast<const PairF*>(F.tsdf + p10);
  s.t11 = *reinterpret_cast<const PairF*>(F.tsdf + p11);
  const PairI w00 = *reinterpret_cast<const PairI*>(F.tsdf_weight + p00);
  const PairI w01 = *reinterpret_cast<const PairI*>(F.tsdf_weight + p01);
  const PairI w10 = *reinterpret_cast<const PairI*>(F.tsdf_weight + p10);
  const PairI w11 = *reinterpret_cast<const PairI*>(F.tsdf_weight + p11);
  s.c00 = lerp(s.t00.a, s.t00.b, s.fz);
  s.c01 = lerp(s.t01.a, s.t01.b, s.fz);
  s.c10 = lerp(s.t10.a, s.t10.b, s.fz);
  s.c11 = lerp(s.t11.a, s.t11.b, s.fz);
  s.c0 = lerp(s.c00, s.c01, s.fy);
  s.c1 = lerp(s.c10, s.c11, s.fy);
  s.value = lerp(s.c0, s.c1, s.fx);
  s.observed = w00.a > 0 && w00.b > 0 && w01.a > 0 && w01.b > 0 && w10.a > 0 && w10.b > 0 && w11.a > 0 && w11.b > 0;
  return s;
}

}  // namespace saf
