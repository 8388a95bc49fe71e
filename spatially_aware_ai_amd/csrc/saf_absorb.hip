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
  PairRows r;
  PairBox b;
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
  const int64_t n = a.b.voxels();
  unsigned long long n_blend = 0, n_copy = 0, n_tblend = 0, n_tcopy = 0;
  for (int64_t i0 = wave * 64; i0 < n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;
    int32_t sv = 0, dv = 0;  // flat voxel indices
    bool copy = false, blend = false, tcopy = false, tblend = false;
    Coef c{0.0f, 0.0f};
    if (i < n) {
      const PairVoxel v = a.b.voxel(i);
      sv = v.sv, dv = v.dv;
      const int32_t ws = a.r.s_weight[sv], tws = a.r.s_tsdf_weight[sv];
      const int32_t wd = a.r.d_weight[dv], twd = a.r.d_tsdf_weight[dv];
      // the TSDF side
      tcopy = tws > 0 && twd <= 0;
      tblend = tws > 0 && twd > 0;
      if (tcopy) {
        a.r.d_tsdf[dv] = a.r.s_tsdf[sv];
        a.r.d_tsdf_weight[dv] = tws;
      } else if (tblend) {
        const Coef t = coef(tws, twd);
        a.r.d_tsdf[dv] = mix(a.r.s_tsdf[sv], a.r.d_tsdf[dv], t.cs, t.cd);
        a.r.d_tsdf_weight[dv] = twd + tws;
      }
      // the feature side: weight and rgb here, the rows below
      copy = ws > 0 && wd <= 0;
      blend = ws > 0 && wd > 0;
      const float* sc = a.r.s_rgb + (int64_t)sv * 3;
      float* dc = a.r.d_rgb + (int64_t)dv * 3;
      if (copy) {
        dc[0] = sc[0];
        dc[1] = sc[1];
        dc[2] = sc[2];
        a.r.d_weight[dv] = ws;
      } else if (blend) {
        c = coef(ws, wd);
        const float r0 = mix(sc[0], dc[0], c.cs, c.cd), r1 = mix(sc[1], dc[1], c.cs, c.cd), r2 = mix(sc[2], dc[2], c.cs, c.cd);
        dc[0] = r0;
        dc[1] = r1;
        dc[2] = r2;
        a.r.d_weight[dv] = wd + ws;
      }
    }
    const unsigned long long mc = __ballot(copy);
    unsigned long long mb = __ballot(blend);
    n_copy += __popcll(mc);
    n_blend += __popcll(mb);
    n_tcopy += __popcll(__ballot(tcopy));
    n_tblend += __popcll(__ballot(tblend));
    copy_rows(mc, sv, dv, lane, a.r);
    while (mb) {
      const int l = __builtin_ctzll(mb);
      mb &= mb - 1;
      const int64_t s = __shfl(sv, l), d = __shfl(dv, l);
      const float cs = __shfl(c.cs, l), cd = __shfl(c.cd, l);  // (the voxel's own lane computed them: the same bits)
      blend_row<KIND>(a.r.d_feat + d * a.r.feat_bytes, a.r.s_feat + s * a.r.feat_bytes, a.r.feat_bytes, a.r.feat_unit, lane, cs, cd);
      if (a.r.s_labels) add_row(a.r.d_labels + d * a.r.label_bytes, a.r.s_labels + s * a.r.label_bytes, a.r.label_bytes, a.r.label_unit, lane);
    }
  }
  add_counts(a.r.counts, lane, n_blend, n_copy, n_tblend, n_tcopy);
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_volume_absorb(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z,
                                 uint64_t* counts, void* stream) {
  if (int rc = check_pair("volume_absorb", src, dst, "the source is only read: two volumes, not one")) return rc;
  // values are computed with, not only copied: the rows are arrays of their element type
  if (int rc = check_computed_pair("volume_absorb", src, dst)) return rc;
  AbsorbArgs a;
  if (!pair_overlap(src, dst, off_x, off_y, off_z, &a.b)) return SAF_OK;  // the boxes share no voxel: nothing to absorb
  a.r = pair_rows(src, dst, counts);
  // (64 voxels per wave and step, 4 waves per workgroup)
  const dim3 grid(grid_1d(a.b.voxels(), 16));
  return dispatch_ft(src->feat_dtype, [&](auto ft) {
    hipLaunchKernelGGL(absorb_kernel<decltype(ft)::value>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("absorb_kernel");
  });
}
