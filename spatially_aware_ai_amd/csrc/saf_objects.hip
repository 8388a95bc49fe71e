// saf_objects.hip -- per-object descriptors of a segmented volume on gfx950 (ABI 6): what flood_fill_3d hands the in-situ
// classifier per object ({"clip_feats", "rgb", "voxels"}, handy_utils.py:400-404) reduced on the device to one row per object --
// voxel count, bounding box, coordinate sum, fused-member count, weight sum, mean colour and mean normalised feature row.
//   * object_init_kernel     : zeroes the accumulators in the workspace, empties the boxes;
//   * object_stats_kernel    : the segmented reduction.  A wave walks fixed chunks of the flat voxel index (z fastest: objects
//                              are runs along z), reads `slot` and `weight` once per voxel, a feature row as 16 bytes per lane and
//                              only for fused members; consecutive members of one object are accumulated in registers and flushed
//                              with 64-bit integer atomics when the slot changes or the chunk ends;
//   * object_finish_kernel   : accumulators -> outputs (every output is written in full).
//
// Determinism (include/saf.h, saf_object_stats): the float outputs are sums of rint(v 2^30), v in [-1, 1], held as 64-bit
// integers -- integer adds commute, so the result does not depend on the grid, the chunking or the order of the atomics -- and one
// division in fp64 rounded to f32.  A row's contribution is a function of the row alone: the lane that holds a column and the order
// of the norm's partial sums are fixed.
#include <math.h>

#include "saf_common.h"
#include "saf_host.h"

#pragma clang fp contract(off)

namespace saf {
namespace {

constexpr int kObjThreads = 256;  // four waves
constexpr int kObjChunk = 512;    // voxels a wave walks before it flushes whatever it holds
constexpr int kObjTile = 512;     // feature columns a wave accumulates: 8 per lane (wider rows: one more grid row per 512 columns)
constexpr float kObjFix = 1073741824.0f;  // 2^30
constexpr double kObjFixD = 1073741824.0;

enum { OBJ_ROWS_NONE = 0, OBJ_VEC_F32 = 1, OBJ_VEC_BF16 = 2, OBJ_SCALAR_F32 = 3, OBJ_SCALAR_BF16 = 4 };

typedef uint32_t obj_u4 __attribute__((ext_vector_type(4)));

struct ObjArgs {
  const int* slot;
  const int* weight;
  const float* rgb;
  const void* feat;
  long long* s_count;  // [K]
  long long* s_fused;  // [K]
  long long* s_weight; // [K]
  long long* s_coord;  // [K,3]
  long long* s_rgb;    // [K,3]
  long long* s_feat;   // [K,D]
  int* s_bbox;         // [K,6]
  int nx, ny, nz;
  int n;  // voxels (< 2^31, checked on the host)
  int K, D;
  int normalize;
  int want_rgb;
};

__device__ __forceinline__ float obj_wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// The 8 values of row `n` that `lane` holds of column tile `tile` (zeros past the row's end).
template <int MODE>
__device__ __forceinline__ void obj_load_tile(const void* feat, int64_t n, int D, int tile, int lane, float (&x)[8]) {
  if (MODE == OBJ_VEC_F32) {
    const v4f_t* row = static_cast<const v4f_t*>(feat) + n * (int64_t)(D >> 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = tile * (kObjTile / 4) + lane + 64 * j;
      v4f_t q = {0.0f, 0.0f, 0.0f, 0.0f};
      if (4 * v < D) q = row[v];
      x[4 * j] = q.x;
      x[4 * j + 1] = q.y;
      x[4 * j + 2] = q.z;
      x[4 * j + 3] = q.w;
    }
  } else if (MODE == OBJ_VEC_BF16) {
    const obj_u4* row = static_cast<const obj_u4*>(feat) + n * (int64_t)(D >> 3);
    const int v = tile * (kObjTile / 8) + lane;
    obj_u4 q = {0u, 0u, 0u, 0u};
    if (8 * v < D) q = row[v];
    x[0] = bf16_lo(q.x);
    x[1] = bf16_hi(q.x);
    x[2] = bf16_lo(q.y);
    x[3] = bf16_hi(q.y);
    x[4] = bf16_lo(q.z);
    x[5] = bf16_hi(q.z);
    x[6] = bf16_lo(q.w);
    x[7] = bf16_hi(q.w);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = tile * kObjTile + lane + 64 * i;
      float q = 0.0f;
      if (c < D) {
        if (MODE == OBJ_SCALAR_F32)
          q = static_cast<const float*>(feat)[n * (int64_t)D + c];
        else
          q = __builtin_bit_cast(float, (uint32_t) static_cast<const uint16_t*>(feat)[n * (int64_t)D + c] << 16);
      }
      x[i] = q;
    }
  }
}

// The column of value i of `lane` in `tile` (the layout obj_load_tile reads).
template <int MODE>
__device__ __forceinline__ int obj_column(int tile, int lane, int i) {
  if (MODE == OBJ_VEC_F32) return 4 * (tile * (kObjTile / 4) + lane + 64 * (i >> 2)) + (i & 3);
  if (MODE == OBJ_VEC_BF16) return 8 * (tile * (kObjTile / 8) + lane) + i;
  return tile * kObjTile + lane + 64 * i;
}

// v in [-1, 1] -> rint(v 2^30); NaN counts as 0, anything outside the range as its nearer end
__device__ __forceinline__ long long obj_fix(float v) {
  if (!(v == v)) v = 0.0f;
  v = fminf(fmaxf(v, -1.0f), 1.0f);
  return (long long)(int)__builtin_rintf(v * kObjFix);
}

__device__ __forceinline__ void obj_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// What a wave holds of the run of members of one object it is walking through.  Everything but feat / rgb is wave-uniform.
struct ObjRun {
  int k;
  int count, fused;
  long long weight;
  long long cx, cy, cz;
  int x0, y0, z0, x1, y1, z1;
  long long rgb;      // lanes 0..2
  long long feat[8];  // the lane's columns of the tile
};

__device__ __forceinline__ void obj_run_reset(ObjRun& r, int k, const ObjArgs& A) {
  r.k = k;
  r.count = 0;
  r.fused = 0;
  r.weight = 0;
  r.cx = r.cy = r.cz = 0;
  r.x0 = A.nx;
  r.y0 = A.ny;
  r.z0 = A.nz;
  r.x1 = r.y1 = r.z1 = -1;
  r.rgb = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.feat[i] = 0;
}

template <int MODE>
__device__ __forceinline__ void obj_run_flush(const ObjRun& r, const ObjArgs& A, int tile, int lane, bool first) {
  if (r.k < 0) return;
  const int64_t k = r.k;
  if (first && r.count > 0) {
    if (lane == 0) {
      obj_add(A.s_count + k, r.count);
      obj_add(A.s_coord + 3 * k, r.cx);
      obj_add(A.s_coord + 3 * k + 1, r.cy);
      obj_add(A.s_coord + 3 * k + 2, r.cz);
      atomicMin(A.s_bbox + 6 * k, r.x0);
      atomicMin(A.s_bbox + 6 * k + 1, r.y0);
      atomicMin(A.s_bbox + 6 * k + 2, r.z0);
      atomicMax(A.s_bbox + 6 * k + 3, r.x1);
      atomicMax(A.s_bbox + 6 * k + 4, r.y1);
      atomicMax(A.s_bbox + 6 * k + 5, r.z1);
      if (r.fused > 0) {
        obj_add(A.s_fused + k, r.fused);
        obj_add(A.s_weight + k, r.weight);
      }
    }
    if (A.want_rgb && lane < 3 && r.rgb != 0) obj_add(A.s_rgb + 3 * k + lane, r.rgb);
  }
  if (MODE != OBJ_ROWS_NONE && r.fused > 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = obj_column<MODE>(tile, lane, i);
      if (c < A.D && r.feat[i] != 0) obj_add(A.s_feat + k * A.D + c, r.feat[i]);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(kObjThreads) void object_stats_kernel(const ObjArgs A) {
  const int lane = (int)threadIdx.x & 63;
  const int tile = (int)blockIdx.y, n_tiles = (int)gridDim.y;
  const bool first = tile == 0;  // the grid row that also keeps the counts, boxes and colours
  const int64_t n_chunks = ((int64_t)A.n + kObjChunk - 1) / kObjChunk;
  const int64_t n_waves = (int64_t)gridDim.x * (kObjThreads / 64);
  const int yz = A.ny * A.nz;
  for (int64_t chunk = (int64_t)blockIdx.x * (kObjThreads / 64) + ((int)threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const int64_t v0 = chunk * kObjChunk;
    const int64_t v1 = v0 + kObjChunk < (int64_t)A.n ? v0 + kObjChunk : (int64_t)A.n;
    ObjRun run;
    obj_run_reset(run, -1, A);
    for (int64_t base = v0; base < v1; base += 64) {
      const int64_t v = base + lane;
      int k = -1, w = 0;
      if (v < v1) {
        k = A.slot[v];
        w = A.weight[v];
      }
      const bool member = (unsigned)k < (unsigned)A.K;  // 0 <= k < K
      unsigned long long mask = __ballot(member);
      if (mask == 0ull) continue;
      const int vi = (int)v;
      const int x = vi / yz, rem = vi - x * yz;
      const int y = rem / A.nz, z = rem - y * A.nz;
      while (mask != 0ull) {
        const int j = __builtin_ctzll(mask);
        mask &= mask - 1ull;
        const int kj = __builtin_amdgcn_readlane(k, j);
        const int wj = __builtin_amdgcn_readlane(w, j);
        if (kj != run.k) {
          obj_run_flush<MODE>(run, A, tile, lane, first);
          obj_run_reset(run, kj, A);
        }
        const bool fused = wj > 0;
        if (first) {
          const int xj = __builtin_amdgcn_readlane(x, j), yj = __builtin_amdgcn_readlane(y, j), zj = __builtin_amdgcn_readlane(z, j);
          run.count += 1;
          run.cx += xj;
          run.cy += yj;
          run.cz += zj;
          run.x0 = xj < run.x0 ? xj : run.x0;
          run.y0 = yj < run.y0 ? yj : run.y0;
          run.z0 = zj < run.z0 ? zj : run.z0;
          run.x1 = xj > run.x1 ? xj : run.x1;
          run.y1 = yj > run.y1 ? yj : run.y1;
          run.z1 = zj > run.z1 ? zj : run.z1;
          if (fused) {
            run.weight += wj;
            if (A.want_rgb && lane < 3) {
              const float c = A.rgb[3 * (base + j) + lane];
              run.rgb += obj_fix(fminf(fmaxf(c, 0.0f), 1.0f));  // .clamp(0, 1) as saf_sample_vertices
            }
          }
        }
        if (fused) {
          run.fused += 1;
          if (MODE != OBJ_ROWS_NONE) {
            const int64_t n = base + j;
            float xs[8];
            obj_load_tile<MODE>(A.feat, n, A.D, tile, lane, xs);
            float ss = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) ss += xs[i] * xs[i];
            for (int t = 0; t < n_tiles; ++t) {  // (rows wider than a tile: the rest of the row, for its norm)
              if (t == tile) continue;
              float ys[8];
              obj_load_tile<MODE>(A.feat, n, A.D, t, lane, ys);
#pragma unroll
              for (int i = 0; i < 8; ++i) ss += ys[i] * ys[i];
            }
            float norm = sqrtf(obj_wave_sum(ss));
            if (A.normalize == SAF_NORM_L2_CLAMP) norm = norm < 0.1f ? 0.1f : norm;
#pragma unroll
            for (int i = 0; i < 8; ++i) run.feat[i] += obj_fix(xs[i] / norm);
          }
        }
      }
    }
    obj_run_flush<MODE>(run, A, tile, lane, first);
  }
}

__global__ __launch_bounds__(256) void object_init_kernel(long long* words, int64_t n_words, int* bbox, int K, int nx, int ny, int nz) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += stride) words[i] = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 6 * (int64_t)K; i += stride) {
    const int c = (int)(i % 6);
    bbox[i] = c == 0 ? nx : c == 1 ? ny : c == 2 ? nz : -1;
  }
}

struct ObjOut {
  int64_t* count;
  int64_t* n_fused;
  int64_t* weight_sum;
  int32_t* bbox;
  int64_t* coord_sum;
  float* rgb_mean;
  float* feat_mean;
};

// S / (2^30 n) in fp64, rounded once to f32
__device__ __forceinline__ float obj_mean(long long s, long long n) {
  return n > 0 ? (float)((double)s / (kObjFixD * (double)n)) : 0.0f;
}

__global__ __launch_bounds__(256) void object_finish_kernel(const ObjArgs A, const ObjOut O) {
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t k = t0; k < A.K; k += stride) {
    O.count[k] = A.s_count[k];
    if (O.n_fused) O.n_fused[k] = A.s_fused[k];
    if (O.weight_sum) O.weight_sum[k] = A.s_weight[k];
#pragma unroll
    for (int c = 0; c < 6; ++c) O.bbox[6 * k + c] = A.s_bbox[6 * k + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (O.coord_sum) O.coord_sum[3 * k + c] = A.s_coord[3 * k + c];
      if (O.rgb_mean) O.rgb_mean[3 * k + c] = obj_mean(A.s_rgb[3 * k + c], A.s_fused[k]);
    }
  }
  if (O.feat_mean) {
    const int64_t total = (int64_t)A.K * A.D;
    for (int64_t i = t0; i < total; i += stride) O.feat_mean[i] = obj_mean(A.s_feat[i], A.s_fused[i / A.D]);
  }
}

size_t object_workspace_bytes(int64_t n_voxels, int64_t K, int64_t D) {
  if (n_voxels < 1 || n_voxels > 0x7fffffffLL || K < 1 || D < 1) return 0;
  const size_t bytes = (size_t)K * (8u * (9u + (size_t)D) + 24u);
  return (bytes + 255) & ~(size_t)255;
}

template <int MODE>
void launch_stats(const ObjArgs& a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL(object_stats_kernel<MODE>, grid, dim3(kObjThreads), 0, s, a);
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" {

size_t saf_object_stats_workspace_bytes(int64_t n_voxels, int32_t n_objects, int32_t feat_dim) {
  return object_workspace_bytes(n_voxels, n_objects, feat_dim);
}

int saf_object_stats(const saf_volume* vol, const int32_t* slot, int32_t n_objects, int32_t normalize, int64_t* count,
                     int64_t* n_fused, int64_t* weight_sum, int32_t* bbox, int64_t* coord_sum, float* rgb_mean, float* feat_mean,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!vol || !slot || !count || !bbox || n_objects < 1)
    return fail(SAF_E_INVALID, "object stats: bad arguments (vol, slot, count and bbox are required; %d objects)", (int)n_objects);
  if (vol->nx < 1 || vol->ny < 1 || vol->nz < 1 || n_voxels(vol) > 0x7fffffffLL || vol->feat_dim < 1 || !vol->weight ||
      (rgb_mean && !vol->rgb) || (feat_mean && !vol->clip_feat))
    return fail(SAF_E_INVALID, "object stats: bad volume (%d x %d x %d voxels, fewer than 2^31 in all; %d channels)", (int)vol->nx,
                (int)vol->ny, (int)vol->nz, (int)vol->feat_dim);
  if (normalize == SAF_NORM_NONE)
    return fail(SAF_E_UNSUPPORTED, "object stats: SAF_NORM_NONE is not offered (raw rows have no bounded range to sum exactly)");
  if (normalize != SAF_NORM_L2 && normalize != SAF_NORM_L2_CLAMP) return fail(SAF_E_INVALID, "object stats: bad normalize %d", (int)normalize);
  if (feat_mean && vol->feat_dtype != SAF_F32 && vol->feat_dtype != SAF_BF16)
    return fail(SAF_E_UNSUPPORTED, "object stats: f32 and bf16 volumes only");
  const int64_t N = n_voxels(vol);
  const int K = n_objects, D = vol->feat_dim;
  const size_t need = object_workspace_bytes(N, K, D);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255))
    return fail(SAF_E_INVALID, "object stats: workspace of %zu bytes, %zu needed on a 256-byte boundary", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);

  ObjArgs a;
  a.slot = slot;
  a.weight = vol->weight;
  a.rgb = vol->rgb;
  a.feat = vol->clip_feat;
  long long* w = static_cast<long long*>(workspace);
  a.s_count = w;
  a.s_fused = w + K;
  a.s_weight = w + 2 * (int64_t)K;
  a.s_coord = w + 3 * (int64_t)K;
  a.s_rgb = w + 6 * (int64_t)K;
  a.s_feat = w + 9 * (int64_t)K;
  const int64_t n_words = 9 * (int64_t)K + (int64_t)K * D;
  a.s_bbox = reinterpret_cast<int*>(w + n_words);
  a.nx = vol->nx;
  a.ny = vol->ny;
  a.nz = vol->nz;
  a.n = (int)N;
  a.K = K;
  a.D = D;
  a.normalize = normalize;
  a.want_rgb = rgb_mean ? 1 : 0;

  {
    const int64_t words = feat_mean ? n_words : 9 * (int64_t)K;
    hipLaunchKernelGGL(object_init_kernel, dim3(grid_1d(words, 8)), dim3(256), 0, s, w, words, a.s_bbox, K, a.nx, a.ny, a.nz);
    int rc = check_launch("object_init_kernel");
    if (rc) return rc;
  }
  {
    const int es = vol->feat_dtype == SAF_BF16 ? 2 : 4;
    const bool vec = ((int64_t)D * es) % 16 == 0 && ((uintptr_t)vol->clip_feat & 15) == 0;
    const int64_t n_chunks = (N + kObjChunk - 1) / kObjChunk;
    const dim3 grid(grid_1d(n_chunks, 8, kObjThreads / 64), feat_mean ? (unsigned)((D + kObjTile - 1) / kObjTile) : 1u);
    if (!feat_mean)
      launch_stats<OBJ_ROWS_NONE>(a, grid, s);
    else if (es == 4)
      vec ? launch_stats<OBJ_VEC_F32>(a, grid, s) : launch_stats<OBJ_SCALAR_F32>(a, grid, s);
    else
      vec ? launch_stats<OBJ_VEC_BF16>(a, grid, s) : launch_stats<OBJ_SCALAR_BF16>(a, grid, s);
    int rc = check_launch("object_stats_kernel");
    if (rc) return rc;
  }
  {
    ObjOut o;
    o.count = count;
    o.n_fused = n_fused;
    o.weight_sum = weight_sum;
    o.bbox = bbox;
    o.coord_sum = coord_sum;
    o.rgb_mean = rgb_mean;
    o.feat_mean = feat_mean;
    const int64_t items = feat_mean ? (int64_t)K * D : (int64_t)K;
    hipLaunchKernelGGL(object_finish_kernel, dim3(grid_1d(items, 8)), dim3(256), 0, s, a, o);
    return check_launch("object_finish_kernel");
  }
}

}  // extern "C"
