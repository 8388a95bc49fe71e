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
  PairRows r;
  PairBox b;
  const int32_t* s_aux;  // NULL: no aux pair
  int32_t* d_aux;
};

// A wave takes 64 consecutive voxels of the FLATTENED overlap box (z fastest, as the volume is laid out): an overlap a few voxels
// deep keeps its lanes busy.  Each lane copies its own voxel's small fields; the ballot names the touched voxels, whose rows
// the whole wave copies one after the other.
__global__ __launch_bounds__(256) void carry_kernel(const CarryArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t n = a.b.voxels();
  unsigned long long n_rows = 0, n_tsdf = 0;
  for (int64_t i0 = wave * 64; i0 < n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;
    int32_t sv = 0, dv = 0;  // flat voxel indices
    bool touched = false, seen = false;
    if (i < n) {
      const PairVoxel v = a.b.voxel(i);
      sv = v.sv, dv = v.dv;
      const int32_t w = a.r.s_weight[sv], tw = a.r.s_tsdf_weight[sv];
      a.r.d_weight[dv] = w;
      a.r.d_tsdf_weight[dv] = tw;
      a.r.d_tsdf[dv] = a.r.s_tsdf[sv];
      const float* sc = a.r.s_rgb + (int64_t)sv * 3;
      float* dc = a.r.d_rgb + (int64_t)dv * 3;
      dc[0] = sc[0];
      dc[1] = sc[1];
      dc[2] = sc[2];
      if (a.s_aux) a.d_aux[dv] = a.s_aux[sv];
      touched = w > 0;
      seen = tw > 0;
    }
    const unsigned long long m = __ballot(touched);
    n_rows += __popcll(m);
    n_tsdf += __popcll(__ballot(seen));
    copy_rows(m, sv, dv, lane, a.r);
  }
  add_counts(a.r.counts, lane, n_rows, n_tsdf);
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
  CarryArgs a;
  if (!pair_overlap(src, dst, off_x, off_y, off_z, &a.b)) return SAF_OK;  // the boxes share no voxel: nothing to carry
  a.r = pair_rows(src, dst, counts);
  a.s_aux = aux_src, a.d_aux = aux_dst;
  // (64 voxels per wave and step, 4 waves per workgroup)
  hipLaunchKernelGGL(carry_kernel, dim3(grid_1d(a.b.voxels(), 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("carry_kernel");
}
