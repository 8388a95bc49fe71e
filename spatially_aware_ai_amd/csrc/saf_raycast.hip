// saf_raycast.hip -- viewing the fused volume from a camera pose on gfx950 (new capability: the reference has no ray cast; its AR
// client, app_unity.py / magicleap2_camera_match.py, is what needs one):
//   * raycast_kernel     : one ray per pixel through the TSDF -- camera depth of the first front-face zero crossing, the voxel
//                          nearest to it and that voxel's colour;
//   * gather_rows_kernel : dst[p, :] = src[index[p], :] (zeros for index < 0) in 16-byte lane accesses: the hit voxels' feature
//                          rows for the existing text-query scans.
//
// Numerics contract of the ray cast (include/saf.h, saf_raycast; tests/raycast_reference.py restates it in NumPy): its reading of
// the TSDF as a field (the grid frame, the pixel's ray, the trilinear sample) has its one C statement in saf_field_dev.h; the
// rest -- the box clip, the march and the hit -- is below, every fp32 operation written on its own, in the order stated there;
// the translation unit is compiled with -ffp-contract=off and divisions are IEEE.
#include <math.h>

#include "saf_field_dev.h"

#pragma clang fp contract(off)

namespace saf {
namespace {

constexpr int kRayThreads = 256;    // four waves: a 16 x 16-pixel block, one 8 x 8 tile per wave
constexpr int kRayBlock = 16;
constexpr int kRayMaxSamples = 65536;  // per ray (a bound on the loop whatever the arguments are)
constexpr int kXcds = 8;

struct RayArgs {
  FieldArgs field;
  const int* weight;
  const float* rgb;
  const float* pose;
  const float* K;
  float* out_depth;
  int* out_voxel;
  float* out_rgb;
  int height, width;
  int tiles_x;
  float step_vox, z_near, z_far;
};

// one slab of the box clip: g(t) = og + t gd within [0, hi]
__device__ __forceinline__ bool clip_axis(float og, float gd, float hi, float& tmin, float& tmax) {
  if (gd != 0.0f) {
    const float t1 = (0.0f - og) / gd;
    const float t2 = (hi - og) / gd;
    tmin = fmaxf(tmin, fminf(t1, t2));
    tmax = fminf(tmax, fmaxf(t1, t2));
    return true;
  }
  return og >= 0.0f && og <= hi;
}

__device__ __forceinline__ int nearest_voxel(float g, int n) {
  int i = (int)__builtin_rintf(g);  // round half to even
  i = i < 0 ? 0 : i;
  return i > n - 1 ? n - 1 : i;
}

__global__ __launch_bounds__(kRayThreads) void raycast_kernel(const RayArgs A) {
  // Blocks are dealt to the XCDs round-robin; the remap gives every XCD one contiguous run of 16 x 16-pixel blocks in raster
  // order (a band of the image), so that neighbouring tiles' taps meet in one L2.  Bijective for any grid size.
  const int nb = (int)gridDim.x, b = (int)blockIdx.x;
  const int per = nb / kXcds, rem = nb % kXcds, xcd = b % kXcds;
  const int blk = xcd * per + (xcd < rem ? xcd : rem) + b / kXcds;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int u = (blk % A.tiles_x) * kRayBlock + (wave & 1) * 8 + (lane & 7);
  const int v = (blk / A.tiles_x) * kRayBlock + (wave >> 1) * 8 + (lane >> 3);
  if (u >= A.width || v >= A.height) return;

  const FieldArgs& F = A.field;
  const GridFrame G = grid_frame(F);
  const float vs = G.vs;
  // the ray in camera z: p(t) = o + t d, d = R (dcx, dcy, 1)
  float dcx, dcy;
  pixel_ray(A.K, u, v, dcx, dcy);
  const float* P = A.pose;
  const float dx = (P[0] * dcx + P[1] * dcy) + P[2];
  const float dy = (P[4] * dcx + P[5] * dcy) + P[6];
  const float dz = (P[8] * dcx + P[9] * dcy) + P[10];
  // in grid coordinates: g(t) = og + t gd
  const float ogx = (P[3] - G.ox) / vs, ogy = (P[7] - G.oy) / vs, ogz = (P[11] - G.oz) / vs;
  const float gdx = dx / vs, gdy = dy / vs, gdz = dz / vs;

  float tmin = A.z_near, tmax = A.z_far;
  bool ok = clip_axis(ogx, gdx, (float)(F.nx - 1), tmin, tmax);
  ok = clip_axis(ogy, gdy, (float)(F.ny - 1), tmin, tmax) && ok;
  ok = clip_axis(ogz, gdz, (float)(F.nz - 1), tmin, tmax) && ok;
  ok = ok && tmin <= tmax;
  ok = ok && is_pinhole(A.K);  // otherwise every pixel is a miss

  const float dmax = fmaxf(fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dy)), __builtin_fabsf(dz));
  const float s = (A.step_vox * vs) / dmax;

  float depth = 0.0f;
  int voxel = -1;
  if (ok && s > 0.0f) {
    float prev_f = 0.0f;
    bool prev_obs = false;
    for (int k = 0; k < kRayMaxSamples; ++k) {
      const float t = tmin + (float)k * s;
      if (!(t <= tmax)) break;
      const FieldSample smp = sample_field(F, ogx + t * gdx, ogy + t * gdy, ogz + t * gdz);
      const float f = smp.value;
      const bool obs = smp.observed;
      if (prev_obs && obs && prev_f > 0.0f && f <= 0.0f) {
        const float t0 = tmin + (float)(k - 1) * s;
        const float ts = t0 + s * (prev_f / (prev_f - f));
        const int vx = nearest_voxel(ogx + ts * gdx, F.nx);
        const int vy = nearest_voxel(ogy + ts * gdy, F.ny);
        const int vz = nearest_voxel(ogz + ts * gdz, F.nz);
        depth = ts;
        voxel = (vx * F.ny + vy) * F.nz + vz;
        break;
      }
      prev_f = f;
      prev_obs = obs;
    }
  }
  const int pix = v * A.width + u;
  A.out_depth[pix] = depth;
  A.out_voxel[pix] = voxel;
  if (A.out_rgb) {
    float r = 0.0f, g = 0.0f, bl = 0.0f;
    if (voxel >= 0 && A.weight[voxel] > 0) {
      r = A.rgb[3 * (int64_t)voxel];
      g = A.rgb[3 * (int64_t)voxel + 1];
      bl = A.rgb[3 * (int64_t)voxel + 2];
    }
    A.out_rgb[3 * (int64_t)pix] = r;
    A.out_rgb[3 * (int64_t)pix + 1] = g;
    A.out_rgb[3 * (int64_t)pix + 2] = bl;
  }
}

// One 16-byte piece of a row per thread; an index outside [0, n_src_rows) gives zeros.
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, int64_t n_src_rows, int64_t row_vecs,
                                                          const int* __restrict__ index, int64_t n_index, uint4* __restrict__ dst) {
  const int64_t total = n_index * row_vecs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i / row_vecs, c = i - p * row_vecs;
    const int64_t r = index[p];
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (r >= 0 && r < n_src_rows) x = src[r * row_vecs + c];
    dst[i] = x;
  }
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" {

int saf_raycast(const saf_volume* vol, const float* pose, const float* K, int32_t height, int32_t width, float step_vox,
                float z_near, float z_far, float* out_depth, int32_t* out_voxel, float* out_rgb, void* stream) {
  if (!vol || !pose || !K || !out_depth || !out_voxel || height <= 0 || width <= 0 || !(step_vox > 0.0f) || !(z_far > z_near))
    return fail(SAF_E_INVALID, "raycast: bad arguments (%d x %d pixels, step_vox = %g, z in [%g, %g])", (int)height, (int)width,
                (double)step_vox, (double)z_near, (double)z_far);
  if (int rc = check_field_volume("raycast", vol, !out_rgb || (vol->rgb && vol->weight))) return rc;
  if (int rc = check_pixel_count("raycast", height, width)) return rc;
  RayArgs a;
  a.field = field_args(vol);
  a.weight = vol->weight;
  a.rgb = vol->rgb;
  a.pose = pose;
  a.K = K;
  a.out_depth = out_depth;
  a.out_voxel = out_voxel;
  a.out_rgb = out_rgb;
  a.height = height;
  a.width = width;
  a.tiles_x = (width + kRayBlock - 1) / kRayBlock;
  a.step_vox = step_vox;
  a.z_near = z_near;
  a.z_far = z_far;
  const int64_t blocks = (int64_t)a.tiles_x * ((height + kRayBlock - 1) / kRayBlock);
  hipLaunchKernelGGL(raycast_kernel, dim3((unsigned)blocks), dim3(kRayThreads), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("raycast_kernel");
}

int saf_gather_rows(const void* src, int64_t n_src_rows, int64_t row_bytes, const int32_t* index, int64_t n_index, void* dst,
                    void* stream) {
  if (!src || !index || !dst || n_src_rows <= 0 || n_index <= 0 || row_bytes <= 0 || row_bytes % 16 != 0 ||
      ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
    return fail(SAF_E_INVALID, "gather rows: bad arguments (%lld source rows of %lld bytes, %lld indices; rows are multiples of 16 "
                "bytes on 16-byte boundaries)", (long long)n_src_rows, (long long)row_bytes, (long long)n_index);
  const int64_t row_vecs = row_bytes / 16;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_1d(n_index * row_vecs, 16)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint4*>(src), n_src_rows, row_vecs, index, n_index, static_cast<uint4*>(dst));
  return check_launch("gather_rows_kernel");
}

}  // extern "C"
