// saf_carve.hip -- saf_free_space_observe and saf_volume_carve: fused voxels that later frames SEE THROUGH are taken out again
// (new capability: the reference's integrate moves such a voxel's TSDF towards +1, clipfusion.py:678-679,
// and leaves its weight, colour, features and label histogram where they were).  Two passes.  The OBSERVE pass classifies every
// touched voxel's centre against every frame of the call exactly as the fuse path does -- saf_common.h's project and nearest_index
// and the sdf lines of saf_fuse.hip's sweep, the same operations on the same values -- and counts, per voxel, the frames that look
// through it (tsdf_valid && !valid: sdf > 1) and the frames that support a surface there (valid: |sdf| <= 1).  The APPLY pass
// decides from the two counts and turns a carved voxel back into the voxel a fresh volume holds: zero bytes everywhere.
#include "saf_common.h"
#include "saf_pair.h"

namespace saf {
namespace {

struct ObserveArgs {
  const int32_t* weight;
  const float *ax, *ay, *az;
  int32_t nx, ny, nz;
  float trunc;
  const float* depth;  // [B,H,W]
  const float* poses;  // [B,4,4]
  const float* K;      // [B,3,3]
  int32_t batch, height, width;
  int32_t* seen;
  int32_t* hit;
};

// A wave owns 64 consecutive voxels of the flattened grid (z fastest) and is their only writer: no atomics.  A wave none of whose
// voxels is touched leaves at once.  The frame loop is wave-uniform: every frame's pose and K are read through uniform addresses
// and its Cam is built once per frame (what depends on the image size alone, once per wave); the two counts stay in registers over
// the call's frames, then one load / add / store per touched lane.  One group of 64 voxels per wave and no loop over groups: every
// store of the kernel comes after its last load.
__global__ __launch_bounds__(256) void observe_kernel(const ObserveArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)a.nx * a.ny * a.nz;  // fewer than 2^31
  const int64_t i = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
  const bool touched = i < n && a.weight[i] > 0;
  if (__ballot(touched) == 0) return;
  const uint32_t ii = i < n ? (uint32_t)i : 0u;
  const uint32_t q = ii / (uint32_t)a.nz, iz = ii - q * (uint32_t)a.nz;
  const uint32_t ix = q / (uint32_t)a.ny, iy = q - ix * (uint32_t)a.ny;
  const float xw = a.ax[ix], yw = a.ay[iy], zw = a.az[iz];
  const float rtrunc = 1.0f / a.trunc;
  const int64_t pixels = (int64_t)a.height * a.width;
  Cam cam = load_cam(a.poses, a.K, a.width, a.height);  // (fw, fh and what follows from them: the same for every frame)
  int32_t n_seen = 0, n_hit = 0;
  for (int f = 0; f < a.batch; ++f) {
    const float* __restrict__ pose = a.poses + (int64_t)f * 16;
    const float* __restrict__ K = a.K + (int64_t)f * 9;
    cam.r00 = pose[0], cam.r01 = pose[1], cam.r02 = pose[2], cam.tx = pose[3];
    cam.r10 = pose[4], cam.r11 = pose[5], cam.r12 = pose[6], cam.ty = pose[7];
    cam.r20 = pose[8], cam.r21 = pose[9], cam.r22 = pose[10], cam.tz = pose[11];
    cam.k00 = K[0], cam.k01 = K[1], cam.k02 = K[2];
    cam.k10 = K[3], cam.k11 = K[4], cam.k12 = K[5];
    cam.k20 = K[6], cam.k21 = K[7], cam.k22 = K[8];
    // saf_fuse.hip's sweep, phases A to C
    const Proj p = project(cam, xw, yw, zw);
    const bool in_view = touched && (fabsf(p.gx) <= 1.0f) && (fabsf(p.gy) <= 1.0f) && (p.z > 0.0f);
    const int pix = in_view ? nearest_index(p.gx, p.gy, cam, a.width) : -1;
    const float depth = pix >= 0 ? a.depth[(int64_t)f * pixels + pix] : 0.0f;
    const float num = depth - p.z;
    const float sdf = num == INFINITY ? INFINITY : div_by_uniform(num, a.trunc, rtrunc);
    const bool valid = in_view && fabsf(sdf) <= 1.0f;
    const bool tsdf_valid = in_view && sdf > -1.0f;
    n_hit += valid ? 1 : 0;
    n_seen += (tsdf_valid && !valid) ? 1 : 0;
  }
  if (touched) {
    a.seen[i] += n_seen;
    a.hit[i] += n_hit;
  }
}

struct CarveArgs {
  float* tsdf;
  int32_t* tsdf_weight;
  int32_t* weight;
  float* rgb;
  unsigned char* feat;
  unsigned char* labels;  // NULL: no label histograms
  const int32_t* seen;
  const int32_t* hit;
  uint8_t* carved;             // NULL: not wanted
  unsigned long long* counts;  // NULL: not counted
  int64_t n, feat_bytes, label_bytes;
  int32_t feat_unit, label_unit;  // bytes per lane and access: saf_pair.h's copy_unit
  int32_t min_views, max_support;
};

// All 64 lanes on one row, `unit` bytes per lane and access: copy_row's shape (saf_pair.h) with zeros for a source.
__device__ __forceinline__ void zero_row(unsigned char* __restrict__ d, int64_t bytes, int unit, int lane) {
  if (unit == 16) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int64_t o = (int64_t)lane * 16; o < bytes; o += 64 * 16) *reinterpret_cast<u32x4*>(d + o) = z;
  } else if (unit == 4) {
    for (int64_t o = (int64_t)lane * 4; o < bytes; o += 64 * 4) *reinterpret_cast<uint32_t*>(d + o) = 0u;
  } else {
    for (int64_t o = (int64_t)lane * 2; o < bytes; o += 64 * 2) *reinterpret_cast<uint16_t*>(d + o) = (uint16_t)0;
  }
}

// A wave takes 64 consecutive voxels.  Each lane decides for its own voxel and zeroes its small fields; a ballot names the carved
// voxels, whose rows the whole wave zeroes one after the other.
__global__ __launch_bounds__(256) void carve_kernel(const CarveArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  unsigned long long n_touched = 0, n_carved = 0, n_supported = 0, n_few = 0;
  for (int64_t i0 = wave * 64; i0 < a.n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;
    bool touched = false, carve = false, supported = false, few = false;
    if (i < a.n) {
      touched = a.weight[i] > 0;
      if (touched) {  // (the evidence of an untouched voxel is not read)
        const int32_t s = a.seen[i], h = a.hit[i];
        const bool enough = s >= a.min_views;
        carve = enough && h <= a.max_support;
        supported = enough && !carve;
        few = !enough && s > 0;
      }
      if (a.carved) a.carved[i] = carve ? 1 : 0;
      if (carve) {
        a.weight[i] = 0;
        a.tsdf_weight[i] = 0;
        a.tsdf[i] = 0.0f;
        float* c = a.rgb + i * 3;
        c[0] = 0.0f, c[1] = 0.0f, c[2] = 0.0f;
      }
    }
    unsigned long long m = __ballot(carve);
    n_touched += __popcll(__ballot(touched));
    n_carved += __popcll(m);
    n_supported += __popcll(__ballot(supported));
    n_few += __popcll(__ballot(few));
    while (m) {
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      const int64_t v = i0 + l;
      zero_row(a.feat + v * a.feat_bytes, a.feat_bytes, a.feat_unit, lane);
      if (a.labels) zero_row(a.labels + v * a.label_bytes, a.label_bytes, a.label_unit, lane);
    }
  }
  add_counts(a.counts, lane, n_touched, n_carved, n_supported, n_few);
}

// What both entries refuse of the volume: the shape, 2^31 voxels or more, sums.
int check_carve_volume(const char* what, const saf_volume* vol) {
  if (!vol) return fail(SAF_E_INVALID, "%s: NULL volume", what);
  if (vol->nx <= 0 || vol->ny <= 0 || vol->nz <= 0)
    return fail(SAF_E_INVALID, "%s: bad volume shape (%d x %d x %d voxels)", what, (int)vol->nx, (int)vol->ny, (int)vol->nz);
  if (n_voxels(vol) >= (int64_t)1 << 31) return fail(SAF_E_INVALID, "%s: a grid of 2^31 voxels or more", what);
  if (vol->accum_mode != SAF_RUNNING_MEAN)
    return fail(SAF_E_UNSUPPORTED, "%s: running means only (accum_mode %d): the sums of a multi-rank job are added by the merge", what,
                (int)vol->accum_mode);
  return SAF_OK;
}

inline bool aligned_to(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_free_space_observe(const saf_volume* vol, const float* depth, int32_t batch, int32_t height, int32_t width,
                                      const float* poses, const float* K, int32_t* seen, int32_t* hit, void* stream) {
  if (int rc = check_carve_volume("free_space_observe", vol)) return rc;
  if (!vol->weight || !vol->axis_x || !vol->axis_y || !vol->axis_z || !depth || !poses || !K || !seen || !hit)
    return fail(SAF_E_INVALID, "free_space_observe: NULL pointer (the volume's weight and axis tables, depth, poses, K, seen, hit)");
  if (batch <= 0 || height <= 0 || width <= 0)
    return fail(SAF_E_INVALID, "free_space_observe: %d frames of %d x %d pixels", (int)batch, (int)height, (int)width);
  if (int rc = check_pixel_count("free_space_observe", height, width)) return rc;
  if (!(vol->trunc > 0.0f) || !std::isfinite(vol->trunc))
    return fail(SAF_E_INVALID, "free_space_observe: truncation distance %g", (double)vol->trunc);
  for (const void* p : {(const void*)vol->weight, (const void*)vol->axis_x, (const void*)vol->axis_y, (const void*)vol->axis_z,
                        (const void*)depth, (const void*)poses, (const void*)K, (const void*)seen, (const void*)hit})
    if (!aligned_to(p, 4)) return fail(SAF_E_INVALID, "free_space_observe: a buffer is not aligned to its element type");
  ObserveArgs a;
  a.weight = vol->weight, a.ax = vol->axis_x, a.ay = vol->axis_y, a.az = vol->axis_z;
  a.nx = vol->nx, a.ny = vol->ny, a.nz = vol->nz, a.trunc = vol->trunc;
  a.depth = depth, a.poses = poses, a.K = K;
  a.batch = batch, a.height = height, a.width = width;
  a.seen = seen, a.hit = hit;
  // (64 voxels per wave, 4 waves per workgroup, one group per wave: fewer than 2^23 workgroups)
  const unsigned blocks = (unsigned)((n_voxels(vol) + 255) / 256);
  hipLaunchKernelGGL(observe_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("observe_kernel");
}

extern "C" int saf_volume_carve(const saf_volume* vol, const int32_t* seen, const int32_t* hit, int32_t min_views, int32_t max_support,
                                uint8_t* carved, uint64_t* counts, void* stream) {
  if (int rc = check_carve_volume("volume_carve", vol)) return rc;
  if (vol->feat_dim <= 0 || vol->n_classes < 0)
    return fail(SAF_E_INVALID, "volume_carve: bad volume shape (%d channels, %d classes)", (int)vol->feat_dim, (int)vol->n_classes);
  if (vol->feat_dtype != SAF_F32 && vol->feat_dtype != SAF_BF16 && vol->feat_dtype != SAF_F16)
    return fail(SAF_E_INVALID, "volume_carve: unknown feature dtype %d", (int)vol->feat_dtype);
  if (!vol->tsdf || !vol->tsdf_weight || !vol->weight || !vol->rgb || !vol->clip_feat || (vol->n_classes > 0 && !vol->labels_one_hot))
    return fail(SAF_E_INVALID, "volume_carve: NULL volume buffer");
  if (!seen || !hit) return fail(SAF_E_INVALID, "volume_carve: NULL evidence (seen, hit)");
  if (min_views < 1 || max_support < 0)
    return fail(SAF_E_INVALID, "volume_carve: min_views %d (at least 1), max_support %d (at least 0)", (int)min_views, (int)max_support);
  for (const void* p : {(const void*)vol->tsdf, (const void*)vol->tsdf_weight, (const void*)vol->weight, (const void*)vol->rgb,
                        (const void*)vol->labels_one_hot, (const void*)seen, (const void*)hit})
    if (!aligned_to(p, 4)) return fail(SAF_E_INVALID, "volume_carve: a buffer is not aligned to its element type");
  if (!aligned_to(vol->clip_feat, vol->feat_dtype == SAF_F32 ? 4 : 2) || !aligned_to(counts, 8))
    return fail(SAF_E_INVALID, "volume_carve: a buffer is not aligned to its element type");
  CarveArgs a;
  a.tsdf = vol->tsdf, a.tsdf_weight = vol->tsdf_weight, a.weight = vol->weight, a.rgb = vol->rgb;
  a.feat = static_cast<unsigned char*>(vol->clip_feat);
  a.n = n_voxels(vol), a.feat_bytes = feat_row_bytes(vol), a.label_bytes = (int64_t)vol->n_classes * 4;
  a.labels = a.label_bytes ? reinterpret_cast<unsigned char*>(vol->labels_one_hot) : nullptr;
  a.seen = seen, a.hit = hit, a.carved = carved;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.feat_unit = copy_unit(a.feat_bytes, a.feat, a.feat);
  a.label_unit = a.label_bytes ? copy_unit(a.label_bytes, a.labels, a.labels) : 4;
  a.min_views = min_views, a.max_support = max_support;
  // (64 voxels per wave and step, 4 waves per workgroup)
  hipLaunchKernelGGL(carve_kernel, dim3(grid_1d(a.n, 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("carve_kernel");
}
