// saf_pair.h -- what the passes over a PAIR of volumes share (saf_carry.hip: the copy; saf_absorb.hip: the blend by weights, both on
// one lattice; saf_coarsen.hip: the weighted mean over blocks of the lattice): the refusals they decide on the host, the overlap box,
// and the row copy of a whole wave.
#pragma once
#include "saf_host.h"

namespace saf {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // (a native vector stays one 16-byte access: saf_merge.hip)

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

// [p, p + bytes) of the two buffers of one name share a byte
inline bool intersect(const void* s, const void* d, int64_t s_bytes, int64_t d_bytes) {
  const uintptr_t sp = (uintptr_t)s, dp = (uintptr_t)d;
  return sp < dp + (uintptr_t)d_bytes && dp < sp + (uintptr_t)s_bytes;
}

// bytes per lane and access that a row pitch and the two bases allow
inline int copy_unit(int64_t row_bytes, const void* s, const void* d) {
  const uintptr_t all = (uintptr_t)row_bytes | (uintptr_t)s | (uintptr_t)d;
  return all % 16 == 0 ? 16 : all % 4 == 0 ? 4 : 2;
}

inline int64_t feat_row_bytes(const saf_volume* v) { return (int64_t)v->feat_dim * (v->feat_dtype == SAF_F32 ? 4 : 2); }

// SAF_E_INVALID for what no pass over a pair takes: a NULL volume or buffer, bad sizes, 2^31 voxels or more, an unknown feature
// dtype, volumes that differ in feat_dim, feat_dtype or n_classes, a destination buffer that shares a byte with the source buffer
// of the same name (`alone`: why the pass `what` needs them apart).
inline int check_pair(const char* what, const saf_volume* src, const saf_volume* dst, const char* alone) {
  if (!src || !dst) return fail(SAF_E_INVALID, "%s: NULL volume", what);
  for (const saf_volume* v : {src, dst}) {
    if (v->nx <= 0 || v->ny <= 0 || v->nz <= 0 || v->feat_dim <= 0 || v->n_classes < 0)
      return fail(SAF_E_INVALID, "%s: bad volume shape (%d x %d x %d voxels, %d channels, %d classes)", what, (int)v->nx, (int)v->ny,
                  (int)v->nz, (int)v->feat_dim, (int)v->n_classes);
    if (n_voxels(v) >= (int64_t)1 << 31) return fail(SAF_E_INVALID, "%s: a grid of 2^31 voxels or more", what);
    if (!v->tsdf || !v->tsdf_weight || !v->weight || !v->rgb || !v->clip_feat || (v->n_classes > 0 && !v->labels_one_hot))
      return fail(SAF_E_INVALID, "%s: NULL volume buffer", what);
  }
  if (src->feat_dtype != SAF_F32 && src->feat_dtype != SAF_BF16 && src->feat_dtype != SAF_F16)
    return fail(SAF_E_INVALID, "%s: unknown feature dtype %d", what, (int)src->feat_dtype);
  if (src->feat_dim != dst->feat_dim || src->feat_dtype != dst->feat_dtype || src->n_classes != dst->n_classes)
    return fail(SAF_E_INVALID, "%s: the volumes differ in feature width, feature dtype or classes (%d/%d/%d and %d/%d/%d)", what,
                (int)src->feat_dim, (int)src->feat_dtype, (int)src->n_classes, (int)dst->feat_dim, (int)dst->feat_dtype, (int)dst->n_classes);
  const int64_t ns = n_voxels(src), nd = n_voxels(dst);
  const int64_t feat_bytes = feat_row_bytes(src), label_bytes = (int64_t)src->n_classes * 4;
  if (intersect(src->tsdf, dst->tsdf, ns * 4, nd * 4) || intersect(src->tsdf_weight, dst->tsdf_weight, ns * 4, nd * 4) ||
      intersect(src->weight, dst->weight, ns * 4, nd * 4) || intersect(src->rgb, dst->rgb, ns * 12, nd * 12) ||
      intersect(src->clip_feat, dst->clip_feat, ns * feat_bytes, nd * feat_bytes) ||
      (label_bytes && intersect(src->labels_one_hot, dst->labels_one_hot, ns * label_bytes, nd * label_bytes)))
    return fail(SAF_E_INVALID, "%s: a destination buffer overlaps its source (%s)", what, alone);
  return SAF_OK;
}

// What the passes that COMPUTE with the rows (saf_absorb.hip, saf_coarsen.hip) refuse on top of check_pair: SAF_E_INVALID for a
// feature or label buffer that is not aligned to its element type (the rows are arrays of that type, not bytes), SAF_E_UNSUPPORTED
// for a volume that holds sums.
inline int check_computed_pair(const char* what, const saf_volume* src, const saf_volume* dst) {
  const int64_t elem = src->feat_dtype == SAF_F32 ? 4 : 2;
  if (((uintptr_t)src->clip_feat | (uintptr_t)dst->clip_feat) % (uintptr_t)elem != 0 ||
      (src->n_classes > 0 && ((uintptr_t)src->labels_one_hot | (uintptr_t)dst->labels_one_hot) % 4 != 0))
    return fail(SAF_E_INVALID, "%s: a feature or label buffer is not aligned to its element type", what);
  if (src->accum_mode != SAF_RUNNING_MEAN || dst->accum_mode != SAF_RUNNING_MEAN)
    return fail(SAF_E_UNSUPPORTED, "%s: running means only (accum_mode %d and %d): the sums of a multi-rank job are added by "
                "the merge", what, (int)src->accum_mode, (int)dst->accum_mode);
  return SAF_OK;
}

// The overlap in destination indices: 0 <= x < dst.n and 0 <= x + off < src.n, per axis (int64: off may be anything).  False: the
// boxes share no voxel.
inline bool pair_overlap(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z, int32_t lo[3],
                         int32_t ext[3]) {
  const int64_t off[3] = {off_x, off_y, off_z}, sn[3] = {src->nx, src->ny, src->nz}, dn[3] = {dst->nx, dst->ny, dst->nz};
  for (int k = 0; k < 3; ++k) {
    const int64_t l = off[k] < 0 ? -off[k] : 0, h = dn[k] < sn[k] - off[k] ? dn[k] : sn[k] - off[k];
    if (h <= l) return false;
    lo[k] = (int32_t)l;
    ext[k] = (int32_t)(h - l);
  }
  return true;
}

}  // namespace saf
