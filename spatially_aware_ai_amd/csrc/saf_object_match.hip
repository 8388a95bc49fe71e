// saf_object_match.hip -- saf_object_overlap: how many voxels every object of one labelling shares with every object of another
// labelling of the SAME lattice (new capability: the reference asks its in-situ classifier whether a newly
// found component "existed", handy_utils.py flood_fill_3d, and this build has no such classifier).  Two int32 slot grids in, a
// dense table of 64-bit counters out; `objects.assign_identities` decides on the host which object is which.
//
// Three launches.  init zeroes an (n_a + 1) x (n_b + 1) table in the workspace -- row n_a / column n_b stand for "no object" --,
// count streams the overlap box once, finish copies the inner block to `pair` and writes the margins as row and column sums.
// Integer atomics only: the result is exact and the same bytes whatever the grid or the scheduling.
#include <algorithm>

#include "saf_host.h"

namespace saf {
namespace {

constexpr int64_t kMaxPairs = (int64_t)1 << 24;  // n_a n_b above this: SAF_E_UNSUPPORTED (a dense table beyond 128 MB)

struct OverlapArgs {
  const int32_t* slot_a;
  const int32_t* slot_b;
  unsigned long long* table;  // [(n_a + 1), (n_b + 1)]
  int32_t ex, ey, ez;         // the overlap box, in voxels
  int32_t lx, ly, lz;         // its low corner in b
  int32_t ox, oy, oz;         // b index + o = a index
  int32_t a_ny, a_nz, b_ny, b_nz;
  int32_t n_a, n_b;
};

__global__ __launch_bounds__(256) void overlap_init_kernel(unsigned long long* __restrict__ table, int64_t words) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) table[i] = 0;
}

// A wave takes kOverlapChunk = 512 consecutive voxels of the FLATTENED overlap box (z fastest, as carry_kernel flattens it,
// saf_carry.hip), 8 per lane in 8 steps of 64: the sixteen slot loads of a lane are in flight together.  Each lane forms the pair
// key row * (n_b + 1) + column per voxel; voxels outside the box and voxels that are no member on either side (most of a volume)
// carry the key of the table's last cell and are dropped by a ballot.  What is left is added per DISTINCT key of the chunk: the
// first live lane's key is broadcast, ballots over the steps not yet exhausted count the voxels that hold it, and that lane adds
// the count with one 64-bit atomic.  Objects are runs along z, so a chunk holds a few keys as a rule; a checkerboard of two
// objects costs two atomics per chunk, not 512.  The loop ends: every turn clears at least the voxel it took the key from.
constexpr int kOverlapSteps = 8, kOverlapChunk = 64 * kOverlapSteps;

__global__ __launch_bounds__(256) void overlap_count_kernel(const OverlapArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t n = (int64_t)a.ex * a.ey * a.ez;  // fewer than 2^31: the overlap lies inside both grids
  const uint32_t ez = (uint32_t)a.ez, ey = (uint32_t)a.ey;
  const int32_t cols = a.n_b + 1, none = a.n_a * cols + a.n_b;  // (n_a + 1)(n_b + 1) <= 2^25 + 2: an int32
  for (int64_t i0 = wave * kOverlapChunk; i0 < n; i0 += n_waves * kOverlapChunk) {
    int32_t key[kOverlapSteps];
    unsigned long long m[kOverlapSteps];
#pragma unroll
    for (int u = 0; u < kOverlapSteps; ++u) {
      const int64_t i = i0 + u * 64 + lane;
      key[u] = none;
      if (i < n) {
        const uint32_t q = (uint32_t)i / ez, z = (uint32_t)i - q * ez;
        const uint32_t x = q / ey, y = q - x * ey;
        const int32_t bx = a.lx + (int32_t)x, by = a.ly + (int32_t)y, bz = a.lz + (int32_t)z;
        const int32_t bv = (bx * a.b_ny + by) * a.b_nz + bz;  // flat voxel indices (both grids hold fewer than 2^31 voxels)
        const int32_t av = ((bx + a.ox) * a.a_ny + (by + a.oy)) * a.a_nz + (bz + a.oz);
        const int32_t sa = a.slot_a[av], sb = a.slot_b[bv];
        const int32_t ka = (uint32_t)sa < (uint32_t)a.n_a ? sa : a.n_a;
        const int32_t kb = (uint32_t)sb < (uint32_t)a.n_b ? sb : a.n_b;
        key[u] = ka * cols + kb;
      }
    }
#pragma unroll
    for (int u = 0; u < kOverlapSteps; ++u) m[u] = __ballot(key[u] != none);
#pragma unroll
    for (int u = 0; u < kOverlapSteps; ++u) {
      while (m[u]) {
        const int l = __builtin_ctzll(m[u]);
        const int32_t k = __shfl(key[u], l);
        unsigned long long count = 0;
#pragma unroll
        for (int v = u; v < kOverlapSteps; ++v) {  // (the steps before u hold no live voxel any more)
          const unsigned long long same = __ballot(key[v] == k);
          count += __popcll(same);
          m[v] &= ~same;
        }
        if (lane == l) atomicAdd(a.table + k, count);
      }
    }
  }
}

// pair = the inner n_a x n_b block (a thread per cell); in_a = row sums over all n_b + 1 columns (a wave per row, lanes along
// the row); in_b = column sums over all n_a + 1 rows (a wave per column, lanes down the column: 64 loads in flight, where a
// thread per column walked its rows one dependent load after the other -- 45 us for a 201 x 201 table).
__global__ __launch_bounds__(256) void overlap_finish_kernel(const unsigned long long* __restrict__ table, int32_t n_a, int32_t n_b,
                                                             int64_t* __restrict__ pair, int64_t* __restrict__ in_a,
                                                             int64_t* __restrict__ in_b) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t cols = (int64_t)n_b + 1, cells = (int64_t)n_a * n_b;
  for (int64_t i = t0; i < cells; i += stride) {
    const int64_t r = i / n_b, c = i - r * n_b;
    pair[i] = (int64_t)table[r * cols + c];
  }
  const int lane = threadIdx.x & 63;
  for (int64_t r = t0 >> 6; r < n_a; r += stride >> 6) {
    unsigned long long s = 0;
    for (int64_t c = lane; c < cols; c += 64) s += table[r * cols + c];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) in_a[r] = (int64_t)s;
  }
  for (int64_t c = t0 >> 6; c < n_b; c += stride >> 6) {
    unsigned long long s = 0;
    for (int64_t r = lane; r <= n_a; r += 64) s += table[r * cols + c];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) in_b[c] = (int64_t)s;
  }
}

size_t overlap_workspace_bytes(int64_t n_a, int64_t n_b) {
  if (n_a < 1 || n_b < 1 || n_a * n_b > kMaxPairs) return 0;
  const size_t bytes = (size_t)(n_a + 1) * (size_t)(n_b + 1) * 8u;
  return (bytes + 255) & ~(size_t)255;
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" {

size_t saf_object_overlap_workspace_bytes(int32_t n_a, int32_t n_b) { return overlap_workspace_bytes(n_a, n_b); }

int saf_object_overlap(const int32_t* slot_a, int32_t ax, int32_t ay, int32_t az, const int32_t* slot_b, int32_t bx, int32_t by,
                       int32_t bz, int32_t off_x, int32_t off_y, int32_t off_z, int32_t n_a, int32_t n_b, int64_t* pair, int64_t* in_a,
                       int64_t* in_b, void* workspace, size_t workspace_bytes, void* stream) {
  if (!slot_a || !slot_b || !pair || !in_a || !in_b)
    return fail(SAF_E_INVALID, "object overlap: NULL pointer (slot_a, slot_b, pair, in_a and in_b are required)");
  if (ax < 1 || ay < 1 || az < 1 || bx < 1 || by < 1 || bz < 1)
    return fail(SAF_E_INVALID, "object overlap: bad grids (%d x %d x %d and %d x %d x %d voxels)", (int)ax, (int)ay, (int)az, (int)bx,
                (int)by, (int)bz);
  if ((int64_t)ax * ay * az >= (int64_t)1 << 31 || (int64_t)bx * by * bz >= (int64_t)1 << 31)
    return fail(SAF_E_INVALID, "object overlap: a grid of 2^31 voxels or more");
  if (n_a < 1 || n_b < 1) return fail(SAF_E_INVALID, "object overlap: %d and %d objects (at least one each)", (int)n_a, (int)n_b);
  if ((int64_t)n_a * n_b > kMaxPairs)
    return fail(SAF_E_UNSUPPORTED, "object overlap: %d x %d objects (the dense table takes at most 2^24 pairs)", (int)n_a, (int)n_b);
  const size_t need = overlap_workspace_bytes(n_a, n_b);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255))
    return fail(SAF_E_INVALID, "object overlap: workspace of %zu bytes, %zu needed on a 256-byte boundary", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* table = static_cast<unsigned long long*>(workspace);
  const int64_t words = ((int64_t)n_a + 1) * ((int64_t)n_b + 1);

  hipLaunchKernelGGL(overlap_init_kernel, dim3(grid_1d(words, 8)), dim3(256), 0, s, table, words);
  int rc = check_launch("overlap_init_kernel");
  if (rc) return rc;

  // the overlap, in b's indices: 0 <= x < b.n and 0 <= x + off < a.n, per axis (int64: off may be anything)
  const int64_t off[3] = {off_x, off_y, off_z}, an[3] = {ax, ay, az}, bn[3] = {bx, by, bz};
  int32_t lo[3], ext[3];
  bool empty = false;
  for (int k = 0; k < 3; ++k) {
    const int64_t l = off[k] < 0 ? -off[k] : 0, h = bn[k] < an[k] - off[k] ? bn[k] : an[k] - off[k];
    if (h <= l) {
      empty = true;  // the boxes share no voxel: the table stays zero
      break;
    }
    lo[k] = (int32_t)l;
    ext[k] = (int32_t)(h - l);
  }
  if (!empty) {
    OverlapArgs a;
    a.slot_a = slot_a, a.slot_b = slot_b, a.table = table;
    a.ex = ext[0], a.ey = ext[1], a.ez = ext[2];
    a.lx = lo[0], a.ly = lo[1], a.lz = lo[2];
    a.ox = off_x, a.oy = off_y, a.oz = off_z;
    a.a_ny = ay, a.a_nz = az, a.b_ny = by, a.b_nz = bz;
    a.n_a = n_a, a.n_b = n_b;
    // (a chunk per wave and turn, 4 waves per workgroup)
    hipLaunchKernelGGL(overlap_count_kernel, dim3(grid_1d((int64_t)ext[0] * ext[1] * ext[2], 16, 4 * kOverlapChunk)), dim3(256), 0, s, a);
    rc = check_launch("overlap_count_kernel");
    if (rc) return rc;
  }
  // (a thread per cell of pair, but no fewer waves than rows + columns where the device has room for them)
  const int64_t finish_items = std::max((int64_t)n_a * n_b, 64 * ((int64_t)n_a + n_b));
  hipLaunchKernelGGL(overlap_finish_kernel, dim3(grid_1d(finish_items, 8)), dim3(256), 0, s, table, n_a, n_b, pair, in_a, in_b);
  return check_launch("overlap_finish_kernel");
}

}  // extern "C"
