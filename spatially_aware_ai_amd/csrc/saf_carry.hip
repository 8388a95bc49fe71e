// saf_carry.hip -- saf_volume_carry: a fused volume carried into another box of the SAME lattice (new
// capability, nothing to mirror in the reference, whose manager fuses every frame of a scan again when the scan grows).  The two
// boxes share origin and voxel size and differ by whole voxels, so the pass is a copy: no value is recomputed, and a voxel both
// boxes contain holds afterwards, byte for byte, what it held before.  One streaming kernel, shaped like pack_rows_kernel
// (saf_merge.hip): 28 bytes of small fields per overlap voxel, and the feature / label rows of the touched voxels only -- a row
// whose voxel has weight 0 is neither read (after a lazy reset it holds the previous scan) nor written.
#include "saf_host.h"

namespace saf {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // (a native vector stays one 16-byte access: saf_merge.hip)

struct CarryArgs {
  const float* s_tsdf;
  const int32_t* s_tsdf_weight;
  const int32_t* s_weight;
  const float* s_rgb;
  const unsigned char* s_feat;
  const unsigned char* s_labels;  // NULL: no label histograms
  const int32_t* s_aux;           // NULL: no aux pair
  float* d_tsdf;
  int32_t* d_tsdf_weight;
  int32_t* d_weight;
  float* d_rgb;
  unsigned char* d_feat;
  unsigned char* d_labels;
  int32_t* d_aux;
  unsigned long long* counts;  // NULL: not counted
  int64_t feat_bytes, label_bytes;  // bytes per row
  int32_t feat_unit, label_unit;    // bytes per lane and access: 16, 4 or 2
  int32_t ex, ey, ez;               // the overlap box, in voxels
  int32_t lx, ly, lz;               // its low corner in the destination
  int32_t ox, oy, oz;               // destination index + o = source index
  int32_t s_ny, s_nz, d_ny, d_nz;
};

// All 64 lanes on one row, `unit` bytes per lane and access (wave-uniform: the branch costs nothing).
__device__ __forceinline__ void copy_row(unsigned char* __restrict__ d, const unsigned char* __restrict__ s, int64_t bytes, int unit,
                                         int lane) {
  if (unit == 16) {
    for (int64_t o = (int64_t)lane * 16; o < bytes; o += 64 * 16) *reinterpret_cast<u32x4*>(d + o) = *reinterpret_cast<const u32x4*>(s + o);
  } else if (unit == 4) {
    for (int64_t o = (int64_t)lane * 4; o < bytes; o += 64 * 4) *reinterpret_cast<uint32_t*>(d + o) = *reinterpret_cast<const uint32_t*>(s + o);
  } else {
    for (int64_t o = (int64_t)lane * 2; o < bytes; o += 64 * 2) *reinterpret_cast<uint16_t*>(d + o) = *reinterpret_cast<const uint16_t*>(s + o);
  }
}

// A wave takes 64 consecutive voxels of the FLATTENED overlap box (z fastest, as the volume is laid out): an overlap a few voxels
// deep keeps its lanes busy.  Each lane copies its own voxel's small fields; the ballot names the touched voxels, whose rows
// the whole wave copies one after the other.
__global__ __launch_bounds__(256) void carry_kernel(const CarryArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t n = (int64_t)a.ex * a.ey * a.ez;  // fewer than 2^31: the overlap lies inside both grids
  const uint32_t ez = (uint32_t)a.ez, ey = (uint32_t)a.ey;
  unsigned long long n_rows = 0, n_tsdf = 0;
  for (int64_t i0 = wave * 64; i0 < n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;
    const bool in = i < n;
    int32_t sv = 0, dv = 0;  // flat voxel indices (both grids hold fewer than 2^31 voxels)
    bool touched = false, seen = false;
    if (in) {
      const uint32_t q = (uint32_t)i / ez, z = (uint32_t)i - q * ez;
      const uint32_t x = q / ey, y = q - x * ey;
      const int32_t dx = a.lx + (int32_t)x, dy = a.ly + (int32_t)y, dz = a.lz + (int32_t)z;
      dv = (dx * a.d_ny + dy) * a.d_nz + dz;
      sv = ((dx + a.ox) * a.s_ny + (dy + a.oy)) * a.s_nz + (dz + a.oz);
      const int32_t w = a.s_weight[sv], tw = a.s_tsdf_weight[sv];
      a.d_weight[dv] = w;
      a.d_tsdf_weight[dv] = tw;
      a.d_tsdf[dv] = a.s_tsdf[sv];
      const float* sc = a.s_rgb + (int64_t)sv * 3;
      float* dc = a.d_rgb + (int64_t)dv * 3;
      dc[0] = sc[0];
      dc[1] = sc[1];
      dc[2] = sc[2];
      if (a.s_aux) a.d_aux[dv] = a.s_aux[sv];
      touched = w > 0;
      seen = tw > 0;
    }
    unsigned long long m = __ballot(touched);
    n_rows += __popcll(m);
    n_tsdf += __popcll(__ballot(seen));
    while (m) {
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      const int64_t s = __shfl(sv, l), d = __shfl(dv, l);
      copy_row(a.d_feat + d * a.feat_bytes, a.s_feat + s * a.feat_bytes, a.feat_bytes, a.feat_unit, lane);
      if (a.s_labels) copy_row(a.d_labels + d * a.label_bytes, a.s_labels + s * a.label_bytes, a.label_bytes, a.label_unit, lane);
    }
  }
  // integer adds: the totals are exact whatever the order
  if (a.counts && lane == 0) {
    if (n_rows) atomicAdd(a.counts + 0, n_rows);
    if (n_tsdf) atomicAdd(a.counts + 1, n_tsdf);
  }
}

// [p, p + bytes) of the two buffers of one name share a byte
bool intersect(const void* s, const void* d, int64_t s_bytes, int64_t d_bytes) {
  const uintptr_t sp = (uintptr_t)s, dp = (uintptr_t)d;
  return sp < dp + (uintptr_t)d_bytes && dp < sp + (uintptr_t)s_bytes;
}

// bytes per lane and access that a row pitch and the two bases allow
int copy_unit(int64_t row_bytes, const void* s, const void* d) {
  const uintptr_t all = (uintptr_t)row_bytes | (uintptr_t)s | (uintptr_t)d;
  return all % 16 == 0 ? 16 : all % 4 == 0 ? 4 : 2;
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_volume_carry(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z,
                                const int32_t* aux_src, int32_t* aux_dst, uint64_t* counts, void* stream) {
  if (!src || !dst) return fail(SAF_E_INVALID, "volume_carry: NULL volume");
  for (const saf_volume* v : {src, dst}) {
    if (v->nx <= 0 || v->ny <= 0 || v->nz <= 0 || v->feat_dim <= 0 || v->n_classes < 0)
      return fail(SAF_E_INVALID, "volume_carry: bad volume shape (%d x %d x %d voxels, %d channels, %d classes)", (int)v->nx, (int)v->ny,
                  (int)v->nz, (int)v->feat_dim, (int)v->n_classes);
    if (n_voxels(v) >= (int64_t)1 << 31) return fail(SAF_E_INVALID, "volume_carry: a grid of 2^31 voxels or more");
    if (!v->tsdf || !v->tsdf_weight || !v->weight || !v->rgb || !v->clip_feat || (v->n_classes > 0 && !v->labels_one_hot))
      return fail(SAF_E_INVALID, "volume_carry: NULL volume buffer");
  }
  if (src->feat_dtype != SAF_F32 && src->feat_dtype != SAF_BF16 && src->feat_dtype != SAF_F16)
    return fail(SAF_E_INVALID, "volume_carry: unknown feature dtype %d", (int)src->feat_dtype);
  if (src->feat_dim != dst->feat_dim || src->feat_dtype != dst->feat_dtype || src->n_classes != dst->n_classes)
    return fail(SAF_E_INVALID, "volume_carry: the volumes differ in feature width, feature dtype or classes (%d/%d/%d and %d/%d/%d)",
                (int)src->feat_dim, (int)src->feat_dtype, (int)src->n_classes, (int)dst->feat_dim, (int)dst->feat_dtype, (int)dst->n_classes);
  if ((aux_src == nullptr) != (aux_dst == nullptr)) return fail(SAF_E_INVALID, "volume_carry: aux_src and aux_dst come as a pair");
  const int64_t ns = n_voxels(src), nd = n_voxels(dst);
  const int64_t feat_bytes = (int64_t)src->feat_dim * (src->feat_dtype == SAF_F32 ? 4 : 2), label_bytes = (int64_t)src->n_classes * 4;
  if (intersect(src->tsdf, dst->tsdf, ns * 4, nd * 4) || intersect(src->tsdf_weight, dst->tsdf_weight, ns * 4, nd * 4) ||
      intersect(src->weight, dst->weight, ns * 4, nd * 4) || intersect(src->rgb, dst->rgb, ns * 12, nd * 12) ||
      intersect(src->clip_feat, dst->clip_feat, ns * feat_bytes, nd * feat_bytes) ||
      (label_bytes && intersect(src->labels_one_hot, dst->labels_one_hot, ns * label_bytes, nd * label_bytes)) ||
      (aux_src && intersect(aux_src, aux_dst, ns * 4, nd * 4)))
    return fail(SAF_E_INVALID, "volume_carry: a destination buffer overlaps its source (the pass works out of place only)");
  // the overlap, in destination indices: 0 <= x < dst.n and 0 <= x + off < src.n, per axis (int64: off may be anything)
  const int64_t off[3] = {off_x, off_y, off_z}, sn[3] = {src->nx, src->ny, src->nz}, dn[3] = {dst->nx, dst->ny, dst->nz};
  int32_t lo[3], ext[3];
  for (int k = 0; k < 3; ++k) {
    const int64_t l = off[k] < 0 ? -off[k] : 0, h = dn[k] < sn[k] - off[k] ? dn[k] : sn[k] - off[k];
    if (h <= l) return SAF_OK;  // the boxes share no voxel: nothing to carry
    lo[k] = (int32_t)l;
    ext[k] = (int32_t)(h - l);
  }
  CarryArgs a;
  a.s_tsdf = src->tsdf, a.s_tsdf_weight = src->tsdf_weight, a.s_weight = src->weight, a.s_rgb = src->rgb;
  a.s_feat = static_cast<const unsigned char*>(src->clip_feat);
  a.s_labels = label_bytes ? reinterpret_cast<const unsigned char*>(src->labels_one_hot) : nullptr;
  a.s_aux = aux_src;
  a.d_tsdf = dst->tsdf, a.d_tsdf_weight = dst->tsdf_weight, a.d_weight = dst->weight, a.d_rgb = dst->rgb;
  a.d_feat = static_cast<unsigned char*>(dst->clip_feat);
  a.d_labels = label_bytes ? reinterpret_cast<unsigned char*>(dst->labels_one_hot) : nullptr;
  a.d_aux = aux_dst;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.feat_bytes = feat_bytes, a.label_bytes = label_bytes;
  a.feat_unit = copy_unit(feat_bytes, a.s_feat, a.d_feat);
  a.label_unit = label_bytes ? copy_unit(label_bytes, a.s_labels, a.d_labels) : 4;
  a.ex = ext[0], a.ey = ext[1], a.ez = ext[2];
  a.lx = lo[0], a.ly = lo[1], a.lz = lo[2];
  a.ox = off_x, a.oy = off_y, a.oz = off_z;
  a.s_ny = src->ny, a.s_nz = src->nz, a.d_ny = dst->ny, a.d_nz = dst->nz;
  // (64 voxels per wave and step, 4 waves per workgroup)
  hipLaunchKernelGGL(carry_kernel, dim3(grid_1d((int64_t)ext[0] * ext[1] * ext[2], 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("carry_kernel");
}
