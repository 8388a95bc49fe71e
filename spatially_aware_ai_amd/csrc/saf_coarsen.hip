// saf_coarsen.hip -- saf_volume_coarsen: a fused volume coarsened by a whole factor f (2, 3 or 4) on block boundaries of its lattice
// (new capability, nothing to mirror in the reference, which fuses every frame again into a coarser grid).
// A coarse voxel is the weighted mean of the f^3 fine voxels it covers -- saf_volume_absorb's blend (saf_absorb.hip) with up to f^3
// sources instead of two: per side (feature side by `weight`, TSDF side by `tsdf_weight`) no contributing child writes zeros to the
// small fields and NO row, one contributing child is a copy of its bytes, and K >= 2 children blend, r = 1 / (float)(sum of counts)
// by IEEE division, c_k = (float)w_k * r, acc = x_1 * c_1, acc = acc + x_k * c_k in ascending fine flat index -- every f32 operation
// written out (the library is built with -ffp-contract=off), so that tests/coarsen_reference.py restates it bit for bit.
#include "saf_common.h"
#include "saf_pair.h"

namespace saf {
namespace {

struct CoarsenArgs {
  PairRows r;
  int32_t s_nx, s_ny, s_nz;         // the fine box
  int32_t d_nx, d_ny, d_nz;         // the coarse box
  int32_t bx, by, bz;               // the fine box's own index of child 0 of coarse voxel 0: f * floor(off / f) - off, in -(f - 1) .. 0
};

constexpr int kLabels = -1;  // combine_rows' fourth element type: int32 counts, summed

// (a wave-uniform lane `l`: one scalar value, and what is derived from it stays in scalar registers)
__device__ __forceinline__ int32_t bcast(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float bcast(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int32_t, v), l));
}

// One step of the stated sum: the first contributing child's product starts it, every later one is added to it.
__device__ __forceinline__ float step(float acc, float x, float c, bool first) {
  const float p = x * c;
  return first ? p : acc + p;
}

// d <- the combination of the rows of the children named by `cm` (bit j: child j, whose fine flat index lane j holds in `fi` and
// whose coefficient it holds in `cf`), children in ascending order.  MODE is SAF_F32 / SAF_BF16 / SAF_F16 (the weighted mean, one
// narrowing at the end) or kLabels (the int32 sum); all 64 lanes work on one row, UNIT bytes per lane.  The loads of up to 8 children
// are issued before their arithmetic; every loop but the lane's own bound is wave-uniform.
template <int MODE, int UNIT>
__device__ __forceinline__ void combine_rows(unsigned char* __restrict__ d, const unsigned char* __restrict__ s, int64_t bytes, int lane,
                                             int32_t fi, float cf, unsigned long long cm) {
  constexpr int NW = UNIT == 16 ? 4 : 1;                                  // 32-bit words per lane and access
  constexpr int NA = (MODE == SAF_F32 || MODE == kLabels) ? NW : 2 * NW;  // values in them
  constexpr bool F16 = MODE == SAF_F16;
  for (int64_t o0 = 0; o0 < bytes; o0 += 64 * UNIT) {
    const int64_t o = o0 + (int64_t)lane * UNIT;
    const bool in = o < bytes;
    float acc[NA];
    uint32_t sum[NW];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < NW; ++k) sum[k] = 0;
    bool first = true;
    unsigned long long m = cm;
    while (m) {
      uint32_t v[8][NW];
      float c[8];
      bool on[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        on[j] = m != 0;
        c[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < NW; ++k) v[j][k] = 0;
        if (on[j]) {
          const int ch = __builtin_ctzll(m);
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
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (on[j]) {
#pragma unroll
          for (int k = 0; k < NW; ++k) {
            if (MODE == kLabels) {
              sum[k] += v[j][k];  // (two's complement: the int32 add)
            } else if (MODE == SAF_F32) {
              acc[k] = step(acc[k], __builtin_bit_cast(float, v[j][k]), c[j], first);
            } else {
              acc[2 * k] = step(acc[2 * k], h16_lo<F16>(v[j][k]), c[j], first);
              acc[NA > 1 ? 2 * k + 1 : 0] = step(acc[NA > 1 ? 2 * k + 1 : 0], h16_hi<F16>(v[j][k]), c[j], first);
            }
          }
          first = false;
        }
      }
    }
    if (in) {
      uint32_t w[NW];
#pragma unroll
      for (int k = 0; k < NW; ++k)
        w[k] = MODE == kLabels ? sum[k] : MODE == SAF_F32 ? __builtin_bit_cast(uint32_t, acc[k]) : pack_h16<F16>(acc[2 * k], acc[NA > 1 ? 2 * k + 1 : 0]);
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

// A wave takes 64 consecutive voxels of the flattened COARSE box (z fastest: children along z are adjacent in the fine box).  Each
// lane handles its own block's small fields, both sides, in two sweeps over its f^3 children (counts first: the coefficients need
// their sum).  A ballot names the blocks with a row to write, which the whole wave takes one after the other: lane j looks up
// child j of that block (f^3 <= 64), a ballot over the children's counts says which contribute, and their fine indices and
// coefficients are read from those lanes -- the same two operations on the same values as in the block's own lane.
template <int KIND, int F>
__global__ __launch_bounds__(256) void coarsen_kernel(const CoarsenArgs a) {
  constexpr int F3 = F * F * F;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t n = (int64_t)a.d_nx * a.d_ny * a.d_nz;  // fewer than 2^31
  const uint32_t dz = (uint32_t)a.d_nz, dy = (uint32_t)a.d_ny;
  const int jx = lane / (F * F), jy = lane / F % F, jz = lane % F;  // the child this lane looks up in the row phase
  unsigned long long n_blend = 0, n_copy = 0, n_tblend = 0, n_tcopy = 0;
  for (int64_t i0 = wave * 64; i0 < n; i0 += n_waves * 64) {
    const int64_t i = i0 + lane;  // the coarse voxel's flat index
    int32_t fx0 = 0, fy0 = 0, fz0 = 0;  // the block's low corner in the fine box's own indices (may lie outside it)
    int32_t kf = 0, kt = 0;             // contributing children per side
    float rf = 0.0f;
    if (i < n) {
      const uint32_t q = (uint32_t)i / dz, z = (uint32_t)i - q * dz;
      const uint32_t x = q / dy, y = q - x * dy;
      fx0 = a.bx + F * (int32_t)x, fy0 = a.by + F * (int32_t)y, fz0 = a.bz + F * (int32_t)z;
      // ---- the counts
      int32_t wsum = 0, wmax = 0, tsum = 0, tmax = 0;
      for (int cx = 0; cx < F; ++cx) {
        const int32_t px = fx0 + cx;
        if ((uint32_t)px >= (uint32_t)a.s_nx) continue;  // children outside the fine box count as empty
        for (int cy = 0; cy < F; ++cy) {
          const int32_t py = fy0 + cy;
          if ((uint32_t)py >= (uint32_t)a.s_ny) continue;
          const int32_t base = (px * a.s_ny + py) * a.s_nz;
#pragma unroll
          for (int cz = 0; cz < F; ++cz) {
            const int32_t pz = fz0 + cz;
            if ((uint32_t)pz >= (uint32_t)a.s_nz) continue;
            const int32_t w = a.r.s_weight[base + pz], tw = a.r.s_tsdf_weight[base + pz];
            if (w > 0) ++kf, wsum += w, wmax = w > wmax ? w : wmax;
            if (tw > 0) ++kt, tsum += tw, tmax = tw > tmax ? tw : tmax;
          }
        }
      }
      // ---- the small fields (IEEE division, hipcc's default for f32, never the hardware reciprocal)
      rf = kf >= 2 ? 1.0f / (float)wsum : 0.0f;
      const float rt = kt >= 2 ? 1.0f / (float)tsum : 0.0f;
      float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, t = 0.0f;
      bool first = true, tfirst = true;
      if (kf > 0 || kt > 0) {
        for (int cx = 0; cx < F; ++cx) {
          const int32_t px = fx0 + cx;
          if ((uint32_t)px >= (uint32_t)a.s_nx) continue;
          for (int cy = 0; cy < F; ++cy) {
            const int32_t py = fy0 + cy;
            if ((uint32_t)py >= (uint32_t)a.s_ny) continue;
            const int32_t base = (px * a.s_ny + py) * a.s_nz;
#pragma unroll
            for (int cz = 0; cz < F; ++cz) {
              const int32_t pz = fz0 + cz;
              if ((uint32_t)pz >= (uint32_t)a.s_nz) continue;
              const int32_t fv = base + pz;
              const int32_t w = a.r.s_weight[fv], tw = a.r.s_tsdf_weight[fv];
              if (w > 0) {  // (the values of a child with count 0 are never read)
                const float* sc = a.r.s_rgb + (int64_t)fv * 3;
                if (kf == 1) {
                  c0 = sc[0], c1 = sc[1], c2 = sc[2];
                } else {
                  const float c = (float)w * rf;
                  c0 = step(c0, sc[0], c, first), c1 = step(c1, sc[1], c, first), c2 = step(c2, sc[2], c, first);
                  first = false;
                }
              }
              if (tw > 0) {
                if (kt == 1) {
                  t = a.r.s_tsdf[fv];
                } else {
                  t = step(t, a.r.s_tsdf[fv], (float)tw * rt, tfirst);
                  tfirst = false;
                }
              }
            }
          }
        }
      }
      float* dc = a.r.d_rgb + i * 3;
      dc[0] = c0, dc[1] = c1, dc[2] = c2;
      a.r.d_weight[i] = wmax;
      a.r.d_tsdf[i] = t;
      a.r.d_tsdf_weight[i] = tmax;
    }
    unsigned long long rows = __ballot(kf > 0);
    n_copy += __popcll(__ballot(kf == 1));
    n_blend += __popcll(__ballot(kf >= 2));
    n_tcopy += __popcll(__ballot(kt == 1));
    n_tblend += __popcll(__ballot(kt >= 2));
    while (rows) {
      const int l = __builtin_ctzll(rows);
      rows &= rows - 1;
      // lane j: child j of lane l's block
      const int32_t px = bcast(fx0, l) + jx, py = bcast(fy0, l) + jy, pz = bcast(fz0, l) + jz;
      const bool ok = lane < F3 && (uint32_t)px < (uint32_t)a.s_nx && (uint32_t)py < (uint32_t)a.s_ny && (uint32_t)pz < (uint32_t)a.s_nz;
      const int32_t fi = ok ? (px * a.s_ny + py) * a.s_nz + pz : 0;
      const int32_t wj = ok ? a.r.s_weight[fi] : 0;
      const unsigned long long cm = __ballot(wj > 0);  // (as many bits as lane l counted: kf)
      const int64_t dv = i0 + l;
      unsigned char* df = a.r.d_feat + dv * a.r.feat_bytes;
      unsigned char* dl = a.r.s_labels ? a.r.d_labels + dv * a.r.label_bytes : nullptr;
      if ((cm & (cm - 1)) == 0) {  // one contributing child: its bytes
        const int64_t sv = bcast(fi, __builtin_ctzll(cm));
        copy_row(df, a.r.s_feat + sv * a.r.feat_bytes, a.r.feat_bytes, a.r.feat_unit, lane);
        if (dl) copy_row(dl, a.r.s_labels + sv * a.r.label_bytes, a.r.label_bytes, a.r.label_unit, lane);
      } else {
        const float cf = (float)wj * bcast(rf, l);
        if (a.r.feat_unit == 16) {
          combine_rows<KIND, 16>(df, a.r.s_feat, a.r.feat_bytes, lane, fi, cf, cm);
        } else if (a.r.feat_unit == 4) {
          combine_rows<KIND, 4>(df, a.r.s_feat, a.r.feat_bytes, lane, fi, cf, cm);
        } else if (KIND != SAF_F32) {  // (an f32 row is never taken 2 bytes at a time: the entry refuses it)
          combine_rows<KIND, 2>(df, a.r.s_feat, a.r.feat_bytes, lane, fi, cf, cm);
        }
        if (dl) {
          if (a.r.label_unit == 16) {
            combine_rows<kLabels, 16>(dl, a.r.s_labels, a.r.label_bytes, lane, fi, cf, cm);
          } else {
            combine_rows<kLabels, 4>(dl, a.r.s_labels, a.r.label_bytes, lane, fi, cf, cm);
          }
        }
      }
    }
  }
  add_counts(a.r.counts, lane, n_blend, n_copy, n_tblend, n_tcopy);
}

// floor(a / f), f > 0
inline int64_t floor_div(int64_t a, int64_t f) { return a >= 0 ? a / f : -((-a + f - 1) / f); }

template <int KIND>
int launch(int factor, dim3 grid, hipStream_t stream, const CoarsenArgs& a) {
  switch (factor) {
    case 2: hipLaunchKernelGGL((coarsen_kernel<KIND, 2>), grid, dim3(256), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((coarsen_kernel<KIND, 3>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((coarsen_kernel<KIND, 4>), grid, dim3(256), 0, stream, a); break;
  }
  return check_launch("coarsen_kernel");
}

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" int saf_volume_coarsen(const saf_volume* src, const saf_volume* dst, int32_t factor, int32_t off_x, int32_t off_y,
                                  int32_t off_z, uint64_t* counts, void* stream) {
  if (int rc = check_pair("volume_coarsen", src, dst, "the pass works out of place only")) return rc;
  if (int rc = check_computed_pair("volume_coarsen", src, dst)) return rc;
  if (factor < 2 || factor > 4) return fail(SAF_E_INVALID, "volume_coarsen: factor %d (2, 3 or 4)", (int)factor);
  const int64_t f = factor, off[3] = {off_x, off_y, off_z}, sn[3] = {src->nx, src->ny, src->nz}, dn[3] = {dst->nx, dst->ny, dst->nz};
  int32_t b[3];
  for (int k = 0; k < 3; ++k) {
    const int64_t lo = floor_div(off[k], f), hi = -floor_div(-(off[k] + sn[k]), f);  // floor(off / f), ceil((off + n) / f)
    if (dn[k] != hi - lo)
      return fail(SAF_E_INVALID, "volume_coarsen: the destination holds %d x %d x %d voxels; axis %d of a %d x %d x %d box at offset "
                  "(%d, %d, %d) coarsens by %d to %lld", (int)dst->nx, (int)dst->ny, (int)dst->nz, k, (int)src->nx, (int)src->ny,
                  (int)src->nz, (int)off_x, (int)off_y, (int)off_z, (int)factor, (long long)(hi - lo));
    b[k] = (int32_t)(f * lo - off[k]);
  }
  CoarsenArgs a;
  a.r = pair_rows(src, dst, counts);
  a.s_nx = src->nx, a.s_ny = src->ny, a.s_nz = src->nz;
  a.d_nx = dst->nx, a.d_ny = dst->ny, a.d_nz = dst->nz;
  a.bx = b[0], a.by = b[1], a.bz = b[2];
  // (64 coarse voxels per wave and step, 4 waves per workgroup)
  const dim3 grid(grid_1d(n_voxels(dst), 16));
  return dispatch_ft(src->feat_dtype, [&](auto ft) { return launch<decltype(ft)::value>(factor, grid, static_cast<hipStream_t>(stream), a); });
}
