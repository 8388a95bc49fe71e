// saf_carry.hip -- saf_volume_carry: a fused volume carried into another box of the SAME lattice (new
// capability, nothing to mirror in the reference, whose manager fuses every frame of a scan again when the scan grows).  The two
// boxes share origin and voxel size and differ by whole voxels, so the pass is a copy: no value is recomputed, and a voxel both
// boxes contain holds afterwards, byte for byte, what it held before.  One streaming kernel, shaped like pack_rows_kernel
// (saf_merge.hip): 28 bytes of small fields per overlap voxel, and the feature / label rows of the touched voxels only -- a row
// whose voxel has weight 0 is neither read (after a lazy reset it holds the previous scan) nor written.
#include "saf_pair.h"

namespace saf {
namespace {

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

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_volume_carry(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z,
                                const int32_t* aux_src, int32_t* aux_dst, uint64_t* counts, void* stream) {
  if (int rc = check_pair("volume_carry", src, dst, "the pass works out of place only")) return rc;
  if ((aux_src == nullptr) != (aux_dst == nullptr)) return fail(SAF_E_INVALID, "volume_carry: aux_src and aux_dst come as a pair");
  if (aux_src && intersect(aux_src, aux_dst, n_voxels(src) * 4, n_voxels(dst) * 4))
    return fail(SAF_E_INVALID, "volume_carry: a destination buffer overlaps its source (the pass works out of place only)");
  const int64_t feat_bytes = feat_row_bytes(src), label_bytes = (int64_t)src->n_classes * 4;
  int32_t lo[3], ext[3];
  if (!pair_overlap(src, dst, off_x, off_y, off_z, lo, ext)) return SAF_OK;  // the boxes share no voxel: nothing to carry
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
