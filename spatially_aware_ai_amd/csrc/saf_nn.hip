// saf_nn.hip -- the label transfer and the scoring of the ScanNet segmentation eval on gfx950
// (reference eval_scannet_segmentation.py:585-601):
//   * nearest_points       : exact nearest reference point of every query point (scipy.spatial.KDTree(pred).query(gt), :585-586)
//                            through a uniform grid: bounding box, cell size and counting sort on the device, then a per-query
//                            search outward by rings of cells;
//   * segmentation_counts  : the confusion matrix and the top-1 / top-k / total counts per class (:589-601, :655-659).
#include <math.h>

#include "saf_common.h"
#include "saf_host.h"

#pragma clang fp contract(off)

namespace saf {
namespace {

constexpr int kNnThreads = 256;
constexpr int kScanItems = 8;                           // cells per thread of the cell-start scan
constexpr int kScanChunk = kNnThreads * kScanItems;     // cells per workgroup of the scan
constexpr int kMaxDim = (1 << 21) + 1;                  // cells per axis at most

struct NnGrid {
  double o[3];    // the grid's origin: the reference points' smallest coordinates
  double hi[3];   // their largest
  double h, inv_h, slack;
  int n[3];
  int bb[6];      // bounding box as order-preserving integers (min x, y, z, max x, y, z) while it is reduced
};

// float -> int with the same order (atomicMin / atomicMax on the bounding box)
__device__ __forceinline__ int ordered(float f) {
  const int b = __builtin_bit_cast(int, f);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float unordered(int b) { return __builtin_bit_cast(float, b >= 0 ? b : b ^ 0x7fffffff); }

__global__ void nn_init_kernel(NnGrid* g) {
  if (threadIdx.x == 0) {
    for (int a = 0; a < 3; ++a) {
      g->bb[a] = 0x7fffffff;
      g->bb[3 + a] = (int)0x80000000;
    }
  }
}

__global__ __launch_bounds__(kNnThreads) void nn_bbox_kernel(const float* __restrict__ ref, int64_t n_ref, NnGrid* g) {
  __shared__ int s_bb[6];
  if (threadIdx.x < 6) s_bb[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : (int)0x80000000;
  __syncthreads();
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n_ref; i += (int64_t)gridDim.x * kNnThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int v = ordered(ref[i * 3 + a]);
      lo[a] = min(lo[a], v);
      hi[a] = max(hi[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(&s_bb[a], lo[a]);
    atomicMax(&s_bb[3 + a], hi[a]);
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&g->bb[threadIdx.x], s_bb[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(&g->bb[threadIdx.x], s_bb[threadIdx.x]);
}

__device__ double grid_cells(const double (&ext)[3], double h, int (&n)[3]) {
  double cells = 1.0;
  for (int a = 0; a < 3; ++a) {
    const double c = fmin(floor(ext[a] / h) + 1.0, (double)kMaxDim);
    n[a] = (int)c;
    cells *= c;
  }
  return cells;
}

// The cell size: the smallest h (to 2^-60 of the box) whose grid has at most `cap` cells.  A flat axis (a plane of mesh vertices)
// gets one cell; non-finite boxes (non-finite input) one cell in all, which keeps every index in bounds.
__global__ void nn_grid_kernel(NnGrid* g, int64_t cap) {
  if (threadIdx.x != 0) return;
  double ext[3], mx = 0.0, mag = 0.0;
  bool finite = true;
  for (int a = 0; a < 3; ++a) {
    const float lo = unordered(g->bb[a]), hi = unordered(g->bb[3 + a]);
    finite = finite && isfinite(lo) && isfinite(hi) && hi >= lo;
    g->o[a] = lo;
    g->hi[a] = hi;
    ext[a] = (double)hi - (double)lo;
    mx = fmax(mx, ext[a]);
    mag = fmax(mag, fmax(fabs((double)lo), fabs((double)hi)));
  }
  int n[3] = {1, 1, 1};
  double h = 1.0;
  if (!finite) {
    for (int a = 0; a < 3; ++a) g->o[a] = g->hi[a] = 0.0;
    mx = mag = 0.0;
  } else if (mx > 0.0) {
    double lo = mx / (double)(kMaxDim - 1), hi = 2.0 * mx;  // hi: one cell per axis
    if (grid_cells(ext, lo, n) <= (double)cap) hi = lo;
    for (int it = 0; it < 64 && hi > lo; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (mid <= lo || mid >= hi) break;
      if (grid_cells(ext, mid, n) <= (double)cap) hi = mid;
      else lo = mid;
    }
    h = hi;
    grid_cells(ext, h, n);
  }
  g->h = h;
  g->inv_h = 1.0 / h;
  // what the cell of a point and the faces of a cell may be off by in fp64 (a few ulps of the coordinates): the search's lower
  // bounds are lowered by it, so a rounding can only make it search more
  g->slack = 1e-12 * (mag + mx + h);
  for (int a = 0; a < 3; ++a) g->n[a] = n[a];
}

__device__ __forceinline__ int cell_axis(double x, double o, double inv_h, int n) {
  const double t = (x - o) * inv_h;
  return t >= 1.0 ? (t < (double)n ? (int)t : n - 1) : 0;  // (NaN: 0)
}
__device__ __forceinline__ int64_t cell_of(const NnGrid& g, float x, float y, float z, int (&c)[3]) {
  c[0] = cell_axis(x, g.o[0], g.inv_h, g.n[0]);
  c[1] = cell_axis(y, g.o[1], g.inv_h, g.n[1]);
  c[2] = cell_axis(z, g.o[2], g.inv_h, g.n[2]);
  return ((int64_t)c[0] * g.n[1] + c[1]) * g.n[2] + c[2];
}

__global__ __launch_bounds__(kNnThreads) void nn_count_kernel(const float* __restrict__ ref, int64_t n_ref, const NnGrid* __restrict__ gp,
                                                              int* __restrict__ count, int* __restrict__ pcell) {
  const NnGrid g = *gp;
  for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n_ref; i += (int64_t)gridDim.x * kNnThreads) {
    int c[3];
    const int64_t cell = cell_of(g, ref[i * 3], ref[i * 3 + 1], ref[i * 3 + 2], c);
    pcell[i] = (int)cell;
    atomicAdd(&count[cell], 1);
  }
}

// exclusive scan of count[0, n) into start[0, n): per-chunk sums, a scan of those in one workgroup, then the chunks
__device__ __forceinline__ int block_exclusive_scan(int v, int* s) {  // over the workgroup; s: kNnThreads ints
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < kNnThreads; o <<= 1) {
    const int add = t >= o ? s[t - o] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const int incl = s[t];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(kNnThreads) void nn_chunk_sums_kernel(const int* __restrict__ count, int64_t n, int* __restrict__ sums) {
  __shared__ int s[kNnThreads];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
  int v = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) v += base + j < n ? count[base + j] : 0;
  const int ex = block_exclusive_scan(v, s);
  if (threadIdx.x == kNnThreads - 1) sums[blockIdx.x] = ex + v;
}

__global__ __launch_bounds__(kNnThreads) void nn_scan_sums_kernel(int* __restrict__ sums, int64_t n_chunks) {
  __shared__ int s[kNnThreads];
  int carry = 0;
  for (int64_t b0 = 0; b0 < n_chunks; b0 += kNnThreads) {
    const int64_t b = b0 + threadIdx.x;
    const int v = b < n_chunks ? sums[b] : 0;
    const int ex = block_exclusive_scan(v, s);
    if (b < n_chunks) sums[b] = carry + ex;
    if (threadIdx.x == kNnThreads - 1) s[0] = ex + v;  // the chunk's total
    __syncthreads();
    carry += s[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kNnThreads) void nn_chunk_scan_kernel(const int* __restrict__ count, int64_t n, const int* __restrict__ sums,
                                                                   int* __restrict__ start) {
  __shared__ int s[kNnThreads];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems], tot = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    v[j] = base + j < n ? count[base + j] : 0;
    tot += v[j];
  }
  int run = sums[blockIdx.x] + block_exclusive_scan(tot, s);
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    if (base + j < n) start[base + j] = run;
    run += v[j];
  }
}

// points into cell order: (x, y, z, index) per point, cell by cell (inside a cell in any order: ties are broken by index)
__global__ __launch_bounds__(kNnThreads) void nn_scatter_kernel(const float* __restrict__ ref, int64_t n_ref, const int* __restrict__ pcell,
                                                                const int* __restrict__ start, int* __restrict__ cursor,
                                                                float4* __restrict__ sorted) {
  for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n_ref; i += (int64_t)gridDim.x * kNnThreads) {
    const int c = pcell[i];
    const int at = start[c] + atomicAdd(&cursor[c], 1);
    sorted[at] = make_float4(ref[i * 3], ref[i * 3 + 1], ref[i * 3 + 2], __builtin_bit_cast(float, (int)i));
  }
}

// One query per thread.  Ring r holds the cells at Chebyshev distance r from the query's (clamped) cell.  A point of a cell not yet
// searched lies beyond one face of the searched block on some axis, and inside the bounding box on the others, so its squared
// distance is at least  gap^2 + sum of the other axes' distances outside the box^2  for the nearest such face: the search stops
// when the best distance is below that for every face with cells behind it (strictly: an equal distance may be a smaller index).
__global__ __launch_bounds__(kNnThreads) void nn_query_kernel(const float* __restrict__ query, int64_t n_query, const NnGrid* __restrict__ gp,
                                                              const int* __restrict__ start, const float4* __restrict__ sorted,
                                                              int* __restrict__ out_index, double* __restrict__ out_dist2) {
  const NnGrid g = *gp;
  for (int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x; i < n_query; i += (int64_t)gridDim.x * kNnThreads) {
    const float qf[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
    int c[3];
    (void)cell_of(g, qf[0], qf[1], qf[2], c);
    const double q[3] = {qf[0], qf[1], qf[2]};
    double out2[3];  // squared distance outside the box on each axis
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double d = fmax(fmax(g.o[a] - q[a], q[a] - g.hi[a]) - g.slack, 0.0);
      out2[a] = d * d;
    }
    double best = INFINITY;
    int bi = 0x7fffffff;
    auto visit = [&](int x, int y, int z) {
      const int64_t cell = ((int64_t)x * g.n[1] + y) * g.n[2] + z;
      const int e = start[cell + 1];
      for (int j = start[cell]; j < e; ++j) {
        const float4 p = sorted[j];
        const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
        const double d2 = dx * dx + dy * dy + dz * dz;
        const int id = __builtin_bit_cast(int, p.w);
        if (d2 < best || (d2 == best && id < bi)) {
          best = d2;
          bi = id;
        }
      }
    };
    for (int r = 0;; ++r) {
      const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.n[0] - 1);
      const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
      const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1);
      for (int x = x0; x <= x1; ++x) {
        const bool xe = x == c[0] - r || x == c[0] + r;
        for (int y = y0; y <= y1; ++y) {
          if (xe || y == c[1] - r || y == c[1] + r) {
            for (int z = z0; z <= z1; ++z) visit(x, y, z);
          } else {
            if (c[2] - r >= 0) visit(x, y, c[2] - r);
            if (r > 0 && c[2] + r < g.n[2]) visit(x, y, c[2] + r);
          }
        }
      }
      double lb = INFINITY;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double others = out2[0] + out2[1] + out2[2] - out2[a];
        if (c[a] - r > 0) {  // cells below the block on this axis
          const double gap = fmax(q[a] - (g.o[a] + (double)(c[a] - r) * g.h) - g.slack, 0.0);
          lb = fmin(lb, gap * gap + others);
        }
        if (c[a] + r < g.n[a] - 1) {  // cells above it
          const double gap = fmax(g.o[a] + (double)(c[a] + r + 1) * g.h - q[a] - g.slack, 0.0);
          lb = fmin(lb, gap * gap + others);
        }
      }
      if (lb == INFINITY || best < lb) break;  // (INFINITY: every cell searched)
    }
    out_index[i] = bi;
    if (out_dist2) out_dist2[i] = best;
  }
}

// ---- scoring counts.  Per workgroup: the class vectors in LDS (and the whole confusion matrix where it fits: up to 120 classes),
// flushed once with 64-bit atomics; past 120 classes the matrix's off-diagonal bins go to global memory directly (its diagonal is
// the top-1 count).  Integer sums: the result does not depend on the order.
constexpr int kCountThreads = 256;
constexpr int kCountFullMax = 120;
constexpr int kCountMaxClasses = 4096;

template <bool FULL>
__global__ __launch_bounds__(kCountThreads) void seg_counts_kernel(const int* __restrict__ gt, const int* __restrict__ pred, int64_t n,
                                                                   int pstride, int topk, int C, unsigned long long* __restrict__ cmat,
                                                                   unsigned long long* __restrict__ top1,
                                                                   unsigned long long* __restrict__ topkc,
                                                                   unsigned long long* __restrict__ total) {
  extern __shared__ int s_cnt[];  // total[C], top1[C], topk[C], (FULL) cmat[C * C]
  int* s_tot = s_cnt;
  int* s_t1 = s_cnt + C;
  int* s_tk = s_cnt + 2 * C;
  int* s_cm = s_cnt + 3 * C;
  const int n_bins = 3 * C + (FULL ? C * C : 0);
  for (int b = threadIdx.x; b < n_bins; b += kCountThreads) s_cnt[b] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kCountThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCountThreads) {
    const int g = gt[i];
    if (g < 0 || g >= C) continue;  // unlabelled (-1) or not a class of the list
    const int* p = pred + i * pstride;
    const int p0 = p[0];
    bool in = false;
    for (int j = 0; j < topk; ++j) in = in || p[j] == g;
    atomicAdd(&s_tot[g], 1);
    if (p0 == g) atomicAdd(&s_t1[g], 1);
    if (in) atomicAdd(&s_tk[g], 1);
    if (p0 >= 0 && p0 < C) {
      if (FULL) atomicAdd(&s_cm[g * C + p0], 1);
      else if (p0 != g) atomicAdd(&cmat[(int64_t)g * C + p0], 1ull);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < C; b += kCountThreads) {
    if (s_tot[b]) atomicAdd(&total[b], (unsigned long long)s_tot[b]);
    if (s_t1[b]) atomicAdd(&top1[b], (unsigned long long)s_t1[b]);
    if (s_tk[b]) atomicAdd(&topkc[b], (unsigned long long)s_tk[b]);
    if (!FULL && s_t1[b]) atomicAdd(&cmat[(int64_t)b * C + b], (unsigned long long)s_t1[b]);
  }
  if (FULL)
    for (int b = threadIdx.x; b < C * C; b += kCountThreads)
      if (s_cm[b]) atomicAdd(&cmat[b], (unsigned long long)s_cm[b]);
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace layout of saf_nearest_points (cap: the most cells a grid may have)
struct NnLayout {
  int64_t cap, n_chunks;
  size_t grid, count, start, sums, pcell, sorted, total;
};
inline NnLayout nn_layout(int64_t n_ref) {
  NnLayout l;
  l.cap = n_ref / 2 > 1 ? n_ref / 2 : 1;
  l.n_chunks = (l.cap + 1 + kScanChunk - 1) / kScanChunk;
  l.grid = 0;
  l.count = align256(sizeof(NnGrid));
  l.start = l.count + align256((size_t)(l.cap + 1) * sizeof(int));
  l.sums = l.start + align256((size_t)(l.cap + 1) * sizeof(int));
  l.pcell = l.sums + align256((size_t)l.n_chunks * sizeof(int));
  l.sorted = l.pcell + align256((size_t)n_ref * sizeof(int));
  l.total = l.sorted + align256((size_t)n_ref * sizeof(float4));
  return l;
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" {

size_t saf_nearest_workspace_bytes(int64_t n_ref, int64_t n_query) {
  (void)n_query;
  return n_ref > 0 ? nn_layout(n_ref).total : 0;
}

int saf_nearest_points(const float* ref, int64_t n_ref, const float* query, int64_t n_query, int32_t* out_index, double* out_dist2,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!ref || n_ref <= 0 || n_ref > 0x7fffffff || n_query < 0 || (n_query > 0 && (!query || !out_index)))
    return fail(SAF_E_INVALID, "nearest points: bad arguments (n_ref = %lld, n_query = %lld)", (long long)n_ref, (long long)n_query);
  if (n_query == 0) return SAF_OK;
  const NnLayout l = nn_layout(n_ref);
  if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255))
    return fail(SAF_E_WORKSPACE, "nearest points: needs %zu bytes of 256-byte aligned workspace", l.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  NnGrid* g = reinterpret_cast<NnGrid*>(w + l.grid);
  int* count = reinterpret_cast<int*>(w + l.count);
  int* start = reinterpret_cast<int*>(w + l.start);
  int* sums = reinterpret_cast<int*>(w + l.sums);
  int* pcell = reinterpret_cast<int*>(w + l.pcell);
  float4* sorted = reinterpret_cast<float4*>(w + l.sorted);
  const size_t count_bytes = (size_t)(l.cap + 1) * sizeof(int);
  if (hipMemsetAsync(count, 0, count_bytes, s) != hipSuccess) return fail(SAF_E_HIP, "hipMemsetAsync(cell counts)");
  hipLaunchKernelGGL(nn_init_kernel, dim3(1), dim3(64), 0, s, g);
  hipLaunchKernelGGL(nn_bbox_kernel, dim3(grid_1d(n_ref, 4, kNnThreads)), dim3(kNnThreads), 0, s, ref, n_ref, g);
  hipLaunchKernelGGL(nn_grid_kernel, dim3(1), dim3(64), 0, s, g, l.cap);
  hipLaunchKernelGGL(nn_count_kernel, dim3(grid_1d(n_ref, 8, kNnThreads)), dim3(kNnThreads), 0, s, ref, n_ref, g, count, pcell);
  // start[0, cap + 1): cells past the grid's own count are empty, so start[cells] = n_ref whatever the grid turned out to be
  hipLaunchKernelGGL(nn_chunk_sums_kernel, dim3((unsigned)l.n_chunks), dim3(kNnThreads), 0, s, count, l.cap + 1, sums);
  hipLaunchKernelGGL(nn_scan_sums_kernel, dim3(1), dim3(kNnThreads), 0, s, sums, l.n_chunks);
  hipLaunchKernelGGL(nn_chunk_scan_kernel, dim3((unsigned)l.n_chunks), dim3(kNnThreads), 0, s, count, l.cap + 1, sums, start);
  if (hipMemsetAsync(count, 0, count_bytes, s) != hipSuccess) return fail(SAF_E_HIP, "hipMemsetAsync(cell cursors)");
  hipLaunchKernelGGL(nn_scatter_kernel, dim3(grid_1d(n_ref, 8, kNnThreads)), dim3(kNnThreads), 0, s, ref, n_ref, pcell, start, count, sorted);
  hipLaunchKernelGGL(nn_query_kernel, dim3(grid_1d(n_query, 16, kNnThreads)), dim3(kNnThreads), 0, s, query, n_query, g, start, sorted, out_index,
                     out_dist2);
  return check_launch("nearest points");
}

int saf_segmentation_counts(const int32_t* gt, const int32_t* pred, int64_t n, int32_t pred_stride, int32_t topk, int32_t n_classes,
                            int64_t* cmat, int64_t* ncorrect_top1, int64_t* ncorrect_topk, int64_t* ntotal, int32_t accumulate,
                            void* stream) {
  if (n < 0 || n_classes <= 0 || n_classes > kCountMaxClasses || topk < 1 || pred_stride < topk || !cmat || !ncorrect_top1 ||
      !ncorrect_topk || !ntotal || (n > 0 && (!gt || !pred)))
    return fail(SAF_E_INVALID, "segmentation counts: bad arguments (n_classes = %d, topk = %d, pred_stride = %d)", n_classes, topk,
                pred_stride);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t vec = (size_t)n_classes * sizeof(int64_t);
  if (!accumulate) {
    if (hipMemsetAsync(cmat, 0, vec * n_classes, s) != hipSuccess || hipMemsetAsync(ncorrect_top1, 0, vec, s) != hipSuccess ||
        hipMemsetAsync(ncorrect_topk, 0, vec, s) != hipSuccess || hipMemsetAsync(ntotal, 0, vec, s) != hipSuccess)
      return fail(SAF_E_HIP, "segmentation counts: hipMemsetAsync");
  }
  if (n == 0) return SAF_OK;
  const bool full = n_classes <= kCountFullMax;
  const size_t shmem = (size_t)(3 * n_classes + (full ? n_classes * n_classes : 0)) * sizeof(int);
  const unsigned blocks = grid_1d(n, 2, kCountThreads * 16);
  auto fn = full ? seg_counts_kernel<true> : seg_counts_kernel<false>;
  if (int rc = allow_lds(fn, shmem)) return rc;
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(kCountThreads), shmem, s, gt, pred, n, (int)pred_stride, (int)topk, (int)n_classes,
                     reinterpret_cast<unsigned long long*>(cmat), reinterpret_cast<unsigned long long*>(ncorrect_top1),
                     reinterpret_cast<unsigned long long*>(ncorrect_topk), reinterpret_cast<unsigned long long*>(ntotal));
  return check_launch("seg_counts_kernel");
}

}  // extern "C"
