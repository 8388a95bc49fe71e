// saf_pair.h -- what the passes over a PAIR of volumes share (saf_carry.hip: the copy; saf_absorb.hip: the blend by weights, both on
// one lattice; saf_coarsen.hip: the weighted mean over blocks of the lattice): the refusals they decide on the host, the shared
// halves of their kernel arguments (PairRows: the buffers; PairBox: the overlap box), and the row copies of a whole wave.
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

// The buffers of both volumes as a kernel reads them, the totals, and how a whole wave takes a row.
struct PairRows {
  const float* s_tsdf;
  const int32_t* s_tsdf_weight;
  const int32_t* s_weight;
  const float* s_rgb;
  const unsigned char* s_feat;
  const unsigned char* s_labels;  // NULL: no label histograms
  float* d_tsdf;
  int32_t* d_tsdf_weight;
  int32_t* d_weight;
  float* d_rgb;
  unsigned char* d_feat;
  unsigned char* d_labels;
  unsigned long long* counts;  // NULL: not counted
  int64_t feat_bytes, label_bytes;  // bytes per row
  int32_t feat_unit, label_unit;    // bytes per lane and access: 16, 4 or 2 (labels: 16 or 4)
};

// The whole wave copies the feature row and the label row of every voxel named in the ballot `m`, one after the other (bit l: the
// voxel whose flat indices lane l holds in `sv` / `dv`).
__device__ __forceinline__ void copy_rows(unsigned long long m, int32_t sv, int32_t dv, int lane, const PairRows& r) {
  while (m) {
    const int l = __builtin_ctzll(m);
    m &= m - 1;
    const int64_t s = __shfl(sv, l), d = __shfl(dv, l);
    copy_row(r.d_feat + d * r.feat_bytes, r.s_feat + s * r.feat_bytes, r.feat_bytes, r.feat_unit, lane);
    if (r.s_labels) copy_row(r.d_labels + d * r.label_bytes, r.s_labels + s * r.label_bytes, r.label_bytes, r.label_unit, lane);
  }
}

// Lane 0 adds the wave's non-zero totals, two or four of them, to `counts` (integer adds: the totals are exact whatever the order).
__device__ __forceinline__ void add_counts(unsigned long long* counts, int lane, unsigned long long t0, unsigned long long t1,
                                           unsigned long long t2 = 0, unsigned long long t3 = 0) {
  if (counts && lane == 0) {
    if (t0) atomicAdd(counts + 0, t0);
    if (t1) atomicAdd(counts + 1, t1);
    if (t2) atomicAdd(counts + 2, t2);
    if (t3) atomicAdd(counts + 3, t3);
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

// (of a pair that check_pair has taken)
inline PairRows pair_rows(const saf_volume* src, const saf_volume* dst, uint64_t* counts) {
  PairRows r;
  r.feat_bytes = feat_row_bytes(src), r.label_bytes = (int64_t)src->n_classes * 4;
  r.s_tsdf = src->tsdf, r.s_tsdf_weight = src->tsdf_weight, r.s_weight = src->weight, r.s_rgb = src->rgb;
  r.s_feat = static_cast<const unsigned char*>(src->clip_feat);
  r.s_labels = r.label_bytes ? reinterpret_cast<const unsigned char*>(src->labels_one_hot) : nullptr;
  r.d_tsdf = dst->tsdf, r.d_tsdf_weight = dst->tsdf_weight, r.d_weight = dst->weight, r.d_rgb = dst->rgb;
  r.d_feat = static_cast<unsigned char*>(dst->clip_feat);
  r.d_labels = r.label_bytes ? reinterpret_cast<unsigned char*>(dst->labels_one_hot) : nullptr;
  r.counts = reinterpret_cast<unsigned long long*>(counts);
  r.feat_unit = copy_unit(r.feat_bytes, r.s_feat, r.d_feat);
  r.label_unit = r.label_bytes ? copy_unit(r.label_bytes, r.s_labels, r.d_labels) : 4;
  return r;
}

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

struct PairVoxel {
  int32_t sv, dv;  // one voxel's flat index in the source and in the destination (both grids hold fewer than 2^31 voxels)
};

// The box two volumes of one lattice share, as a kernel walks it.
struct PairBox {
  int32_t ex, ey, ez;  // the overlap box, in voxels
  int32_t lx, ly, lz;  // its low corner in the destination
  int32_t ox, oy, oz;  // destination index + o = source index
  int32_t s_ny, s_nz, d_ny, d_nz;

  // fewer than 2^31: the overlap lies inside both grids
  __host__ __device__ int64_t voxels() const { return (int64_t)ex * ey * ez; }

  // voxel `i` of the FLATTENED box (z fastest, as the volumes are laid out)
  __device__ __forceinline__ PairVoxel voxel(int64_t i) const {
    const uint32_t q = (uint32_t)i / (uint32_t)ez, z = (uint32_t)i - q * (uint32_t)ez;
    const uint32_t x = q / (uint32_t)ey, y = q - x * (uint32_t)ey;
    const int32_t dx = lx + (int32_t)x, dy = ly + (int32_t)y, dz = lz + (int32_t)z;
    const int32_t dv = (dx * d_ny + dy) * d_nz + dz;
    return PairVoxel{((dx + ox) * s_ny + (dy + oy)) * s_nz + (dz + oz), dv};
  }
};

// The overlap in destination indices: 0 <= x < dst.n and 0 <= x + off < src.n, per axis (int64: off may be anything).  False: the
// boxes share no voxel.
inline bool pair_overlap(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z, PairBox* b) {
  const int64_t off[3] = {off_x, off_y, off_z}, sn[3] = {src->nx, src->ny, src->nz}, dn[3] = {dst->nx, dst->ny, dst->nz};
  int32_t lo[3], ext[3];
  for (int k = 0; k < 3; ++k) {
    const int64_t l = off[k] < 0 ? -off[k] : 0, h = dn[k] < sn[k] - off[k] ? dn[k] : sn[k] - off[k];
    if (h <= l) return false;
    lo[k] = (int32_t)l;
    ext[k] = (int32_t)(h - l);
  }
  *b = PairBox{ext[0], ext[1], ext[2], lo[0], lo[1], lo[2], off_x, off_y, off_z, src->ny, src->nz, dst->ny, dst->nz};
  return true;
}

}  // namespace saf
