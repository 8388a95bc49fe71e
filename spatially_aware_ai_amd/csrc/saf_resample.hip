// saf_resample.hip -- saf_volume_resample: a fused volume resampled onto ANY other lattice under a rigid transform (rotated, shifted
// by a fraction of a voxel, finer, coarser by any factor; new capability, nothing to mirror in the reference,
// which fuses every frame again into the other grid).  A pull resample: every destination voxel looks up the eight source voxels
// around its own centre and blends the observed ones by their trilinear weights, renormalised -- per side (feature side by `weight`,
// TSDF side by `tsdf_weight`) a voxel whose contributing corners cover less than `min_cover` of the trilinear weight is not observed
// (zeros to the small fields and NO row), one contributing corner is a copy of its bytes, and K >= 2 corners blend, r = 1 / S by
// IEEE division, c_k = t_k * r, acc = x_1 * c_1, acc = acc + x_k * c_k in ascending corner index -- every f32 operation written out
// (the library is built with -ffp-contract=off), so that tests/resample_reference.py restates it bit for bit.
// combine_rows, bcast and step are PRIVATE COPIES of saf_coarsen.hip's (without the label sum: a label row here is copied from the
// heaviest corner): moving them into saf_pair.h would change the text coarsen's and absorb's objects are compiled from.
#include "saf_common.h"
#include "saf_pair.h"

namespace saf {
namespace {

struct ResampleArgs {
  PairRows r;
  int32_t s_nx, s_ny, s_nz;  // the source box
  int32_t d_nx, d_ny, d_nz;  // the destination box
  float m[12];               // destination local index -> continuous source local index, row-major 3 x 4
  float min_cover;
};

// (a wave-uniform lane `l`: one scalar value, and what is derived from it stays in scalar registers)
__device__ __forceinline__ int32_t bcast(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float bcast(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int32_t, v), l));
}

// One step of the stated sum: the first contributing corner's product starts it, every later one is added to it.
__device__ __forceinline__ float step(float acc, float x, float c, bool first) {
  const float p = x * c;
  return first ? p : acc + p;
}

// p_a of the statement: four roundings, no FMA.
__device__ __forceinline__ float axis_p(const float* m, float x, float y, float z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

// One axis of a voxel's footprint: the lower corner's index and the two weights along the axis, a[0] of the lower corner.
struct Axis {
  int32_t i;
  float a0, a1;
};
__device__ __forceinline__ Axis axis_of(float p) {
  const float fl = floorf(p);
  const float f = p - fl;  // ((float)(int)floorf(p) is floorf(p): |p| is far below 2^31)
  return Axis{(int32_t)fl, 1.0f - f, f};
}

// Corner k = 4 dx + 2 dy + dz of a footprint: whether it lies in the source box, its flat index there (0 if not) and its weight.
struct Corner {
  bool in;
  int32_t sv;
  float t;
};
__device__ __forceinline__ Corner corner_of(const ResampleArgs& a, const Axis& x, const Axis& y, const Axis& z, int k) {
  const int dx = (k >> 2) & 1, dy = (k >> 1) & 1, dz = k & 1;
  const int32_t px = x.i + dx, py = y.i + dy, pz = z.i + dz;
  Corner c;
  c.in = (uint32_t)px < (uint32_t)a.s_nx && (uint32_t)py < (uint32_t)a.s_ny && (uint32_t)pz < (uint32_t)a.s_nz;
  c.sv = c.in ? (px * a.s_ny + py) * a.s_nz + pz : 0;
  c.t = ((dx ? x.a1 : x.a0) * (dy ? y.a1 : y.a0)) * (dz ? z.a1 : z.a0);
  return c;
}

// d <- the blend of the rows of the corners named by `cm` (bit j: corner j, whose source flat index lane j holds in `fi` and whose
// coefficient it holds in `cf`), corners in ascending order.  MODE is SAF_F32 / SAF_BF16 / SAF_F16 (one narrowing at the end); all
// 64 lanes work on one row, UNIT bytes per lane.  The loads of all (up to 8) corners are issued before their arithmetic; every loop
// but the lane's own bound is wave-uniform.
template <int MODE, int UNIT>
__device__ __forceinline__ void combine_rows(unsigned char* __restrict__ d, const unsigned char* __restrict__ s, int64_t bytes, int lane,
                                             int32_t fi, float cf, uint32_t cm) {
  constexpr int NW = UNIT == 16 ? 4 : 1;            // 32-bit words per lane and access
  constexpr int NA = MODE == SAF_F32 ? NW : 2 * NW;  // values in them
  constexpr bool F16 = MODE == SAF_F16;
  for (int64_t o0 = 0; o0 < bytes; o0 += 64 * UNIT) {
    const int64_t o = o0 + (int64_t)lane * UNIT;
    const bool in = o < bytes;
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0f;
    uint32_t v[8][NW];
    float c[8];
    bool on[8];
    uint32_t m = cm;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      on[j] = m != 0;
      c[j] = 0.0f;
#pragma unroll
      for (int k = 0; k < NW; ++k) v[j][k] = 0;
      if (on[j]) {
        const int ch = __builtin_ctz(m);
        m &= m - 1;
        const unsigned char* p = s + (int64_t)bcast(fi, ch) * bytes + o;
        c[j] = bcast(cf, ch);
        if (in) {
          if (UNIT == 16) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(p);
            v[j][0] = q.x, v[j][NW > 1 ? 1 : 0] = q.y, v[j][NW > 2 ? 2 : 0] = q.z, v[j][NW > 3 ? 3 : 0] = q.w;
          } else if (UNIT == 4) {
            v[j][0] = *reinterpret_cast<const uint32_t*>(p);
          } else {
            v[j][0] = *reinterpret_cast<const uint16_t*>(p);
          }
        }
      }
    }
    bool first = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (on[j]) {
#pragma unroll
        for (int k = 0; k < NW; ++k) {
          if (MODE == SAF_F32) {
            acc[k] = step(acc[k], __builtin_bit_cast(float, v[j][k]), c[j], first);
          } else {
            acc[2 * k] = step(acc[2 * k], h16_lo<F16>(v[j][k]), c[j], first);
            acc[NA > 1 ? 2 * k + 1 : 0] = step(acc[NA > 1 ? 2 * k + 1 : 0], h16_hi<F16>(v[j][k]), c[j], first);
          }
        }
        first = false;
      }
    }
    if (in) {
      uint32_t w[NW];
#pragma unroll
      for (int k = 0; k < NW; ++k)
        w[k] = MODE == SAF_F32 ? __builtin_bit_cast(uint32_t, acc[k]) : pack_h16<F16>(acc[2 * k], acc[NA > 1 ? 2 * k + 1 : 0]);
      if (UNIT == 16) {
        u32x4 q;
        q.x = w[0], q.y = w[NW > 1 ? 1 : 0], q.z = w[NW > 2 ? 2 : 0], q.w = w[NW > 3 ? 3 : 0];
        *reinterpret_cast<u32x4*>(d + o) = q;
      } else if (UNIT == 4) {
        *reinterpret_cast<uint32_t*>(d + o) = w[0];
      } else {
        *reinterpret_cast<uint16_t*>(d + o) = (uint16_t)(w[0] & 0xffffu);
      }
    }
  }
}

// What one side of a voxel's footprint comes to: the contributing corners (bit k), their count's maximum, and 1 / S (K >= 2).
struct Side {
  uint32_t mask;  // 0: the side is not observed here (no contributing corner, or they cover less than min_cover)
  int32_t wmax;
  float r;
};
__device__ __forceinline__ Side gate(uint32_t mask, float s, int32_t wmax, float min_cover) {
  Side o;
  const bool seen = mask != 0 && s >= min_cover;
  o.mask = seen ? mask : 0;
  o.wmax = seen ? wmax : 0;
  o.r = (o.mask & (o.mask - 1)) ? 1.0f / s : 0.0f;  // (IEEE division, hipcc's default for f32, never the hardware reciprocal)
  return o;
}

// A wave takes 64 consecutive voxels of the flattened DESTINATION box (z fastest).  Each lane handles its own voxel's small fields,
// both sides, in two sweeps over its eight corners (counts first: the coefficients need S).  A ballot names the voxels with a row
// to write, which the whole wave takes one after the other: the footprint (three indices, three fractions), the contributing
// corners and 1 / S are read from the owning lane, lane j < 8 forms corner j from them -- the same operations on the same values as
// in the owning lane -- and the rows' loads are issued before their arithmetic.
template <int KIND>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t n = (int64_t)a.d_nx * a.d_ny * a.d_nz;  // fewer than 2^31
  const uint32_t dz = (uint32_t)a.d_nz, dy = (uint32_t)a.d_ny;
  unsigned long long n_blend = 0, n_copy = 0, n_tblend = 0, n_tcopy = 0;
  for (int64_t i0 = wave * 64; i0 < n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;  // the destination voxel's flat index
    Axis X{0, 0.0f, 0.0f}, Y{0, 0.0f, 0.0f}, Z{0, 0.0f, 0.0f};
    Side sf{0, 0, 0.0f}, st{0, 0, 0.0f};
    int32_t best = 0;  // the feature side's heaviest contributing corner, the lowest on a tie: its label row is taken
    if (i < n) {
      const uint32_t q = (uint32_t)i / dz, z = (uint32_t)i - q * dz;
      const uint32_t x = q / dy, y = q - x * dy;
      const float xf = (float)x, yf = (float)y, zf = (float)z;
      const float px = axis_p(a.m + 0, xf, yf, zf), py = axis_p(a.m + 4, xf, yf, zf), pz = axis_p(a.m + 8, xf, yf, zf);
      // (compared in float, before any conversion to an integer)
      const bool any = !(px < -1.0f || px >= (float)a.s_nx || py < -1.0f || py >= (float)a.s_ny || pz < -1.0f || pz >= (float)a.s_nz);
      float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, t = 0.0f;
      if (any) {
        X = axis_of(px), Y = axis_of(py), Z = axis_of(pz);
        // ---- the counts
        uint32_t fm = 0, tm = 0;
        int32_t wmax = 0, tmax = 0;
        float s_f = 0.0f, s_t = 0.0f, t_best = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const Corner c = corner_of(a, X, Y, Z, k);
          if (c.in && c.t > 0.0f) {
            const int32_t w = a.r.s_weight[c.sv], tw = a.r.s_tsdf_weight[c.sv];
            if (w > 0) {
              s_f = fm ? s_f + c.t : c.t;
              if (!fm || c.t > t_best) t_best = c.t, best = c.sv;
              fm |= 1u << k;
              wmax = w > wmax ? w : wmax;
            }
            if (tw > 0) {
              s_t = tm ? s_t + c.t : c.t;
              tm |= 1u << k;
              tmax = tw > tmax ? tw : tmax;
            }
          }
        }
        sf = gate(fm, s_f, wmax, a.min_cover), st = gate(tm, s_t, tmax, a.min_cover);
        // ---- the small fields
        bool first = true, tfirst = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const Corner c = corner_of(a, X, Y, Z, k);
          if (sf.mask >> k & 1) {  // (the values of a corner that does not contribute are never read)
            const float* sc = a.r.s_rgb + (int64_t)c.sv * 3;
            if (sf.r == 0.0f) {
              c0 = sc[0], c1 = sc[1], c2 = sc[2];
            } else {
              const float cf = c.t * sf.r;
              c0 = step(c0, sc[0], cf, first), c1 = step(c1, sc[1], cf, first), c2 = step(c2, sc[2], cf, first);
              first = false;
            }
          }
          if (st.mask >> k & 1) {
            if (st.r == 0.0f) {
              t = a.r.s_tsdf[c.sv];
            } else {
              t = step(t, a.r.s_tsdf[c.sv], c.t * st.r, tfirst);
              tfirst = false;
            }
          }
        }
      }
      float* dc = a.r.d_rgb + i * 3;
      dc[0] = c0, dc[1] = c1, dc[2] = c2;
      a.r.d_weight[i] = sf.wmax;
      a.r.d_tsdf[i] = t;
      a.r.d_tsdf_weight[i] = st.wmax;
    }
    const bool blend = (sf.mask & (sf.mask - 1)) != 0, tblend = (st.mask & (st.mask - 1)) != 0;
    unsigned long long rows = __ballot(sf.mask != 0);
    n_copy += __popcll(__ballot(sf.mask != 0 && !blend));
    n_blend += __popcll(__ballot(blend));
    n_tcopy += __popcll(__ballot(st.mask != 0 && !tblend));
    n_tblend += __popcll(__ballot(tblend));
    while (rows) {
      const int l = __builtin_ctzll(rows);
      rows &= rows - 1;
      const uint32_t cm = (uint32_t)bcast((int32_t)sf.mask, l);
      const int64_t dv = i0 + l;
      unsigned char* df = a.r.d_feat + dv * a.r.feat_bytes;
      if (a.r.s_labels) {  // the heaviest contributing corner's histogram: votes are not summed over corners
        const int64_t lv = bcast(best, l);
        copy_row(a.r.d_labels + dv * a.r.label_bytes, a.r.s_labels + lv * a.r.label_bytes, a.r.label_bytes, a.r.label_unit, lane);
      }
      if ((cm & (cm - 1)) == 0) {  // one contributing corner: its bytes (it is the heaviest one)
        const int64_t sv = bcast(best, l);
        copy_row(df, a.r.s_feat + sv * a.r.feat_bytes, a.r.feat_bytes, a.r.feat_unit, lane);
      } else {
        // lane j: corner j of lane l's footprint
        const Axis lx{bcast(X.i, l), bcast(X.a0, l), bcast(X.a1, l)}, ly{bcast(Y.i, l), bcast(Y.a0, l), bcast(Y.a1, l)},
            lz{bcast(Z.i, l), bcast(Z.a0, l), bcast(Z.a1, l)};
        const Corner c = corner_of(a, lx, ly, lz, lane & 7);
        const int32_t fi = (lane < 8 && (cm >> lane & 1)) ? c.sv : 0;
        const float cf = c.t * bcast(sf.r, l);
        if (a.r.feat_unit == 16) {
          combine_rows<KIND, 16>(df, a.r.s_feat, a.r.feat_bytes, lane, fi, cf, cm);
        } else if (a.r.feat_unit == 4) {
          combine_rows<KIND, 4>(df, a.r.s_feat, a.r.feat_bytes, lane, fi, cf, cm);
        } else if (KIND != SAF_F32) {  // (an f32 row is never taken 2 bytes at a time: the entry refuses it)
          combine_rows<KIND, 2>(df, a.r.s_feat, a.r.feat_bytes, lane, fi, cf, cm);
        }
      }
    }
  }
  add_counts(a.r.counts, lane, n_blend, n_copy, n_tblend, n_tcopy);
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_volume_resample(const saf_volume* src, const saf_volume* dst, const float* m12, float min_cover, uint64_t* counts,
                                   void* stream) {
  if (int rc = check_pair("volume_resample", src, dst, "the pass works out of place only")) return rc;
  if (int rc = check_computed_pair("volume_resample", src, dst)) return rc;
  if (!m12) return fail(SAF_E_INVALID, "volume_resample: NULL matrix");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(m12[k])) return fail(SAF_E_INVALID, "volume_resample: entry %d of the matrix is not finite", k);
  if (!(min_cover > 0.0f && min_cover <= 1.0f))
    return fail(SAF_E_INVALID, "volume_resample: min_cover %g (more than 0, at most 1)", (double)min_cover);
  ResampleArgs a;
  a.r = pair_rows(src, dst, counts);
  a.s_nx = src->nx, a.s_ny = src->ny, a.s_nz = src->nz;
  a.d_nx = dst->nx, a.d_ny = dst->ny, a.d_nz = dst->nz;
  for (int k = 0; k < 12; ++k) a.m[k] = m12[k];
  a.min_cover = min_cover;
  // (64 destination voxels per wave and step, 4 waves per workgroup)
  const dim3 grid(grid_1d(n_voxels(dst), 16));
  return dispatch_ft(src->feat_dtype, [&](auto ft) {
    hipLaunchKernelGGL((resample_kernel<decltype(ft)::value>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("resample_kernel");
  });
}
