// saf_absorb.hip -- saf_volume_absorb: a second fused volume of the SAME lattice blended into this one by weights (DESIGN.md
// section 4.20; new capability, nothing to mirror in the reference).  Mapping and overlap are saf_volume_carry's (saf_carry.hip);
// where carry copies, this pass decides per voxel and side (feature side by `weight`, TSDF side by `tsdf_weight`): a source count of
// 0 writes nothing, a destination count of 0 takes the source's bytes (the destination's old row is not read: after a deferred clear
// it is stale), and two positive counts blend, x' = xs * (ws * r) + xd * (wd * r) with r = 1 / (ws + wd) by IEEE division -- every
// f32 operation written out (the library is built with -ffp-contract=off), so that tests/absorb_reference.py restates it bit for bit.
#include "saf_common.h"
#include "saf_pair.h"

namespace saf {
namespace {

struct AbsorbArgs {
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
  int32_t ex, ey, ez;               // the overlap box, in voxels
  int32_t lx, ly, lz;               // its low corner in the destination
  int32_t ox, oy, oz;               // destination index + o = source index
  int32_t s_ny, s_nz, d_ny, d_nz;
};

// The two coefficients of a blend of counts ws, wd > 0: cs = ws * r, cd = wd * r, r = RN(1 / (float)(ws + wd)).
struct Coef {
  float cs, cd;
};
__device__ __forceinline__ Coef coef(int32_t ws, int32_t wd) {
  const float r = 1.0f / (float)(wd + ws);  // IEEE division (hipcc's default for f32), never the hardware reciprocal
  return Coef{(float)ws * r, (float)wd * r};
}
// two separately rounded products, one rounded sum
__device__ __forceinline__ float mix(float xs, float xd, float cs, float cd) { return xs * cs + xd * cd; }

// One element type behind one name: KIND is SAF_F32, SAF_BF16 or SAF_F16.
template <int KIND>
__device__ __forceinline__ uint32_t mix_word(uint32_t s, uint32_t d, float cs, float cd) {
  if (KIND == SAF_F32) return __builtin_bit_cast(uint32_t, mix(__builtin_bit_cast(float, s), __builtin_bit_cast(float, d), cs, cd));
  constexpr bool F16 = KIND == SAF_F16;
  return pack_h16<F16>(mix(h16_lo<F16>(s), h16_lo<F16>(d), cs, cd), mix(h16_hi<F16>(s), h16_hi<F16>(d), cs, cd));
}
template <int KIND>
__device__ __forceinline__ u32x4 mix_quad(u32x4 s, u32x4 d, float cs, float cd) {
  u32x4 o;
  o.x = mix_word<KIND>(s.x, d.x, cs, cd);
  o.y = mix_word<KIND>(s.y, d.y, cs, cd);
  o.z = mix_word<KIND>(s.z, d.z, cs, cd);
  o.w = mix_word<KIND>(s.w, d.w, cs, cd);
  return o;
}

// d <- s * cs + d * cd over one feature row.  The 16-byte form takes two steps of the row at once and issues the loads of both
// rows before any arithmetic: 512 f32 channels are four 16-byte loads per lane in flight.
template <int KIND>
__device__ __forceinline__ void blend_row(unsigned char* __restrict__ d, const unsigned char* __restrict__ s, int64_t bytes, int unit,
                                          int lane, float cs, float cd) {
  if (unit == 16) {
    for (int64_t o = (int64_t)lane * 16; o < bytes; o += 2 * 64 * 16) {
      const int64_t o1 = o + 64 * 16;
      const bool two = o1 < bytes;
      const u32x4 s0 = *reinterpret_cast<const u32x4*>(s + o), d0 = *reinterpret_cast<const u32x4*>(d + o);
      u32x4 s1 = s0, d1 = d0;
      if (two) {
        s1 = *reinterpret_cast<const u32x4*>(s + o1);
        d1 = *reinterpret_cast<const u32x4*>(d + o1);
      }
      *reinterpret_cast<u32x4*>(d + o) = mix_quad<KIND>(s0, d0, cs, cd);
      if (two) *reinterpret_cast<u32x4*>(d + o1) = mix_quad<KIND>(s1, d1, cs, cd);
    }
  } else if (unit == 4) {
    for (int64_t o = (int64_t)lane * 4; o < bytes; o += 64 * 4)
      *reinterpret_cast<uint32_t*>(d + o) = mix_word<KIND>(*reinterpret_cast<const uint32_t*>(s + o), *reinterpret_cast<const uint32_t*>(d + o), cs, cd);
  } else if (KIND != SAF_F32) {  // one 16-bit element per lane (an f32 row is never taken 2 bytes at a time: the entry refuses it)
    for (int64_t o = (int64_t)lane * 2; o < bytes; o += 64 * 2) {
      const uint32_t w = mix_word<KIND>(*reinterpret_cast<const uint16_t*>(s + o), *reinterpret_cast<const uint16_t*>(d + o), cs, cd);
      *reinterpret_cast<uint16_t*>(d + o) = (uint16_t)(w & 0xffffu);
    }
  }
}

// d <- d + s over one label histogram row (int32 counts).
__device__ __forceinline__ void add_row(unsigned char* __restrict__ d, const unsigned char* __restrict__ s, int64_t bytes, int unit, int lane) {
  if (unit == 16) {
    for (int64_t o = (int64_t)lane * 16; o < bytes; o += 64 * 16) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(s + o), b = *reinterpret_cast<const u32x4*>(d + o);
      *reinterpret_cast<u32x4*>(d + o) = a + b;  // (two's complement: the int32 add)
    }
  } else {
    for (int64_t o = (int64_t)lane * 4; o < bytes; o += 64 * 4)
      *reinterpret_cast<uint32_t*>(d + o) = *reinterpret_cast<const uint32_t*>(s + o) + *reinterpret_cast<const uint32_t*>(d + o);
  }
}

// carry_kernel's shape (saf_carry.hip): a wave takes 64 consecutive voxels of the FLATTENED overlap box; each lane handles its own
// voxel's small fields, both sides; two ballots name the rows to copy and the rows to blend, which the whole wave takes one after
// the other.  A destination voxel belongs to exactly one lane of one wave: the update in place needs no ordering between waves.
template <int KIND>
__global__ __launch_bounds__(256) void absorb_kernel(const AbsorbArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t n = (int64_t)a.ex * a.ey * a.ez;  // fewer than 2^31: the overlap lies inside both grids
  const uint32_t ez = (uint32_t)a.ez, ey = (uint32_t)a.ey;
  unsigned long long n_blend = 0, n_copy = 0, n_tblend = 0, n_tcopy = 0;
  for (int64_t i0 = wave * 64; i0 < n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;
    int32_t sv = 0, dv = 0;  // flat voxel indices (both grids hold fewer than 2^31 voxels)
    bool copy = false, blend = false, tcopy = false, tblend = false;
    Coef c{0.0f, 0.0f};
    if (i < n) {
      const uint32_t q = (uint32_t)i / ez, z = (uint32_t)i - q * ez;
      const uint32_t x = q / ey, y = q - x * ey;
      const int32_t dx = a.lx + (int32_t)x, dy = a.ly + (int32_t)y, dz = a.lz + (int32_t)z;
      dv = (dx * a.d_ny + dy) * a.d_nz + dz;
      sv = ((dx + a.ox) * a.s_ny + (dy + a.oy)) * a.s_nz + (dz + a.oz);
      const int32_t ws = a.s_weight[sv], tws = a.s_tsdf_weight[sv];
      const int32_t wd = a.d_weight[dv], twd = a.d_tsdf_weight[dv];
      // the TSDF side
      tcopy = tws > 0 && twd <= 0;
      tblend = tws > 0 && twd > 0;
      if (tcopy) {
        a.d_tsdf[dv] = a.s_tsdf[sv];
        a.d_tsdf_weight[dv] = tws;
      } else if (tblend) {
        const Coef t = coef(tws, twd);
        a.d_tsdf[dv] = mix(a.s_tsdf[sv], a.d_tsdf[dv], t.cs, t.cd);
        a.d_tsdf_weight[dv] = twd + tws;
      }
      // the feature side: weight and rgb here, the rows below
      copy = ws > 0 && wd <= 0;
      blend = ws > 0 && wd > 0;
      const float* sc = a.s_rgb + (int64_t)sv * 3;
      float* dc = a.d_rgb + (int64_t)dv * 3;
      if (copy) {
        dc[0] = sc[0];
        dc[1] = sc[1];
        dc[2] = sc[2];
        a.d_weight[dv] = ws;
      } else if (blend) {
        c = coef(ws, wd);
        const float r0 = mix(sc[0], dc[0], c.cs, c.cd), r1 = mix(sc[1], dc[1], c.cs, c.cd), r2 = mix(sc[2], dc[2], c.cs, c.cd);
        dc[0] = r0;
        dc[1] = r1;
        dc[2] = r2;
        a.d_weight[dv] = wd + ws;
      }
    }
    unsigned long long mc = __ballot(copy), mb = __ballot(blend);
    n_copy += __popcll(mc);
    n_blend += __popcll(mb);
    n_tcopy += __popcll(__ballot(tcopy));
    n_tblend += __popcll(__ballot(tblend));
    while (mc) {
      const int l = __builtin_ctzll(mc);
      mc &= mc - 1;
      const int64_t s = __shfl(sv, l), d = __shfl(dv, l);
      copy_row(a.d_feat + d * a.feat_bytes, a.s_feat + s * a.feat_bytes, a.feat_bytes, a.feat_unit, lane);
      if (a.s_labels) copy_row(a.d_labels + d * a.label_bytes, a.s_labels + s * a.label_bytes, a.label_bytes, a.label_unit, lane);
    }
    while (mb) {
      const int l = __builtin_ctzll(mb);
      mb &= mb - 1;
      const int64_t s = __shfl(sv, l), d = __shfl(dv, l);
      const float cs = __shfl(c.cs, l), cd = __shfl(c.cd, l);  // (the voxel's own lane computed them: the same bits)
      blend_row<KIND>(a.d_feat + d * a.feat_bytes, a.s_feat + s * a.feat_bytes, a.feat_bytes, a.feat_unit, lane, cs, cd);
      if (a.s_labels) add_row(a.d_labels + d * a.label_bytes, a.s_labels + s * a.label_bytes, a.label_bytes, a.label_unit, lane);
    }
  }
  // integer adds: the totals are exact whatever the order
  if (a.counts && lane == 0) {
    if (n_blend) atomicAdd(a.counts + 0, n_blend);
    if (n_copy) atomicAdd(a.counts + 1, n_copy);
    if (n_tblend) atomicAdd(a.counts + 2, n_tblend);
    if (n_tcopy) atomicAdd(a.counts + 3, n_tcopy);
  }
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_volume_absorb(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z,
                                 uint64_t* counts, void* stream) {
  if (int rc = check_pair("volume_absorb", src, dst, "the source is only read: two volumes, not one")) return rc;
  // values are computed with, not only copied: the rows are arrays of their element type
  if (int rc = check_computed_pair("volume_absorb", src, dst)) return rc;
  const int64_t feat_bytes = feat_row_bytes(src), label_bytes = (int64_t)src->n_classes * 4;
  int32_t lo[3], ext[3];
  if (!pair_overlap(src, dst, off_x, off_y, off_z, lo, ext)) return SAF_OK;  // the boxes share no voxel: nothing to absorb
  AbsorbArgs a;
  a.s_tsdf = src->tsdf, a.s_tsdf_weight = src->tsdf_weight, a.s_weight = src->weight, a.s_rgb = src->rgb;
  a.s_feat = static_cast<const unsigned char*>(src->clip_feat);
  a.s_labels = label_bytes ? reinterpret_cast<const unsigned char*>(src->labels_one_hot) : nullptr;
  a.d_tsdf = dst->tsdf, a.d_tsdf_weight = dst->tsdf_weight, a.d_weight = dst->weight, a.d_rgb = dst->rgb;
  a.d_feat = static_cast<unsigned char*>(dst->clip_feat);
  a.d_labels = label_bytes ? reinterpret_cast<unsigned char*>(dst->labels_one_hot) : nullptr;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.feat_bytes = feat_bytes, a.label_bytes = label_bytes;
  a.feat_unit = copy_unit(feat_bytes, a.s_feat, a.d_feat);
  a.label_unit = label_bytes ? copy_unit(label_bytes, a.s_labels, a.d_labels) : 4;
  a.ex = ext[0], a.ey = ext[1], a.ez = ext[2];
  a.lx = lo[0], a.ly = lo[1], a.lz = lo[2];
  a.ox = off_x, a.oy = off_y, a.oz = off_z;
  a.s_ny = src->ny, a.s_nz = src->nz, a.d_ny = dst->ny, a.d_nz = dst->nz;
  // (64 voxels per wave and step, 4 waves per workgroup)
  const dim3 grid(grid_1d((int64_t)ext[0] * ext[1] * ext[2], 16));
  return dispatch_ft(src->feat_dtype, [&](auto ft) {
    hipLaunchKernelGGL(absorb_kernel<decltype(ft)::value>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("absorb_kernel");
  });
}
