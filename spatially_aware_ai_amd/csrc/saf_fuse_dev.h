// saf_fuse_dev.h -- device-side building blocks shared by the per-frame pipeline (saf_fuse.hip) and the
// windowed path (saf_window.hip): kernel descriptors, the bilinear blend arithmetic, the rgb / weight / label
// side of one valid voxel, and the host-side profiler pair.  Everything lives in an anonymous namespace: each
// translation unit gets its own copy.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <optional>

#include "saf_common.h"
#include "saf_host.h"

#pragma clang fp contract(off)

// Pool of event pairs; opaque to callers (include/saf.h).
struct saf_profiler {
  struct Pair {
    hipEvent_t a, b;
    int cls;
  };
  Pair* pairs;
  int capacity, used;
  int stride;  // record only frames whose index within the call is a multiple of this
};

namespace saf {

// element type of a volume's feature rows: fp32, or one of the two 16-bit types (same row layout: 8 channels per 16 bytes)
enum { kE16None = 0, kE16Bf16 = 1, kE16Half = 2 };

// kernel-side descriptors (POD, passed by value; shared by both translation units)
struct KVol {
  int nx, ny, nz, D, n_classes, accum, e16;  // e16: kE16None / kE16Bf16 / kE16Half
  uint32_t N;
  float trunc;
  const float *ax, *ay, *az;
  float* tsdf;
  int* tsdf_w;
  int* weight;
  float* rgb;
  float* feat;
  int* labels;
  FastDiv div_nz, div_ny;
};

// The row kernels' one compile-time choice -- the rows' element type x the accumulation rule x the direction --, with exactly the
// kinds that are built.  A seventh is added HERE: an enumerator, its answers in row_traits, its volumes in row_kind_of, its case
// in dispatch_row_kind; the kernels and pickers below then see it.
enum class RowKind { MeanF32, SumF32, MeanBf16, SumBf16, MeanF16, UndoF32 };
struct RowTraits {
  bool sum;     // sums (SAF_SUM), not running means
  bool rows16;  // 16-bit rows: a 16-byte unit holds 8 channels ...
  bool half;    // ... of IEEE half, not bfloat16
  bool undo;    // the kernel runs backwards: the frames leave the rows
  int esz;      // bytes per stored channel
};
constexpr RowTraits row_traits(RowKind k) {
  const bool rows16 = k == RowKind::MeanBf16 || k == RowKind::SumBf16 || k == RowKind::MeanF16;
  return {k == RowKind::SumF32 || k == RowKind::SumBf16, rows16, k == RowKind::MeanF16, k == RowKind::UndoF32, rows16 ? 2 : 4};
}
// The kind of a volume's rows in a direction, or none: fp16 rows hold no sums, and only the f32 running mean is built backwards.
// The ONE mapping of (e16, accum, undo) to kernels: every picker and every refusal of a combination asks it.
inline std::optional<RowKind> row_kind_of(const KVol& kv, bool undo) {
  const bool sum = kv.accum == SAF_SUM;
  if (undo) return (kv.e16 || sum) ? std::nullopt : std::optional<RowKind>(RowKind::UndoF32);
  if (kv.e16 == kE16Half) return sum ? std::nullopt : std::optional<RowKind>(RowKind::MeanF16);
  if (kv.e16) return sum ? RowKind::SumBf16 : RowKind::MeanBf16;
  return sum ? RowKind::SumF32 : RowKind::MeanF32;
}
// One template argument from a run-time kind, as dispatch_dtype (saf_host.h): f(std::integral_constant<RowKind, K>{}).
template <typename F>
auto dispatch_row_kind(RowKind k, F&& f) {
  switch (k) {
    case RowKind::SumF32: return f(std::integral_constant<RowKind, RowKind::SumF32>{});
    case RowKind::MeanBf16: return f(std::integral_constant<RowKind, RowKind::MeanBf16>{});
    case RowKind::SumBf16: return f(std::integral_constant<RowKind, RowKind::SumBf16>{});
    case RowKind::MeanF16: return f(std::integral_constant<RowKind, RowKind::MeanF16>{});
    case RowKind::UndoF32: return f(std::integral_constant<RowKind, RowKind::UndoF32>{});
    default: return f(std::integral_constant<RowKind, RowKind::MeanF32>{});
  }
}

struct KFrame {
  int H, W, npy, npx, rgb_bilinear;
  const float *depth, *rgb, *pose, *K, *label_map;
};

namespace {

FastDiv make_fastdiv(uint32_t d) {
  // q = (n * mul) >> shift is exact for every n < 2^31: with L = ceil(log2 d), S = 31 + L and
  // mul = ceil(2^S / d), the error term e = mul*d - 2^S is < d <= 2^L, so n*e < 2^S.
  uint32_t L = 0;
  while ((1ull << L) < d) ++L;
  FastDiv f;
  f.shift = 31 + L;
  f.mul = (uint32_t)(((1ull << f.shift) + d - 1) / d);
  f.d = d;
  f.pad = 0;
  return f;
}

__device__ __forceinline__ void voxel_coords(const KVol& v, uint32_t n, int& ix, int& iy, int& iz) {
  uint32_t t = fdiv(n, v.div_nz);
  iz = (int)(n - t * (uint32_t)v.nz);
  uint32_t x = fdiv(t, v.div_ny);
  iy = (int)(t - x * (uint32_t)v.ny);
  ix = (int)x;
}

// ------------------------------------------------------------------------------------------
// fuse: gather + running-mean RMW of the valid voxel rows
// ------------------------------------------------------------------------------------------
template <int VEC>
struct VecT;
template <>
struct VecT<4> {
  using type = float4;
};
template <>
struct VecT<1> {
  using type = float;
};

__device__ __forceinline__ float4 lerp_taps(float4 a, float4 b, float4 c, float4 d, const Bilin& w) {
  // (nw_val*nw + ne_val*ne) + sw_val*sw + se_val*se, left to right (GridSamplerKernel.cpp)
  float4 r;
  r.x = ((a.x * w.nw + b.x * w.ne) + c.x * w.sw) + d.x * w.se;
  r.y = ((a.y * w.nw + b.y * w.ne) + c.y * w.sw) + d.y * w.se;
  r.z = ((a.z * w.nw + b.z * w.ne) + c.z * w.sw) + d.z * w.se;
  r.w = ((a.w * w.nw + b.w * w.ne) + c.w * w.sw) + d.w * w.se;
  return r;
}
__device__ __forceinline__ float lerp_taps(float a, float b, float c, float d, const Bilin& w) {
  return ((a * w.nw + b * w.ne) + c * w.sw) + d * w.se;
}
__device__ __forceinline__ float4 blend(float4 s, float4 old, float a, float b, bool sum) {
  float4 r;
  if (sum) {
    r.x = old.x + s.x; r.y = old.y + s.y; r.z = old.z + s.z; r.w = old.w + s.w;
  } else {
    // clip_feat.T * a + self.clip_feat[valid] * b          clipfusion.py:720
    r.x = s.x * a + old.x * b; r.y = s.y * a + old.y * b;
    r.z = s.z * a + old.z * b; r.w = s.w * a + old.w * b;
  }
  return r;
}
__device__ __forceinline__ float blend(float s, float old, float a, float b, bool sum) {
  return sum ? old + s : s * a + old * b;
}

// The blend turned round (saf_unfuse_frames): a sample leaves a running mean.  r = 1 / new_weight, b = weight * r:
// old * b - s * r, two rounded products and one rounded difference (no FMA: contraction is off in these units).  r == 0 stands
// for new_weight == 0: the voxel returns to its constructed state, exact zeros whatever the sample holds.
__device__ __forceinline__ float unblend(float s, float old, float r, float b) { return r == 0.0f ? 0.0f : old * b - s * r; }
__device__ __forceinline__ float4 unblend(float4 s, float4 old, float r, float b) {
  return make_float4(unblend(s.x, old.x, r, b), unblend(s.y, old.y, r, b), unblend(s.z, old.z, r, b), unblend(s.w, old.w, r, b));
}

struct Taps {
  int o_nw, o_ne, o_sw, o_se;  // tap positions in [0, P]; P = the zero column (outside the map)
};
__device__ __forceinline__ Taps tap_offsets(const Bilin& b, int npx, int npy) {
  const bool x0 = b.x0 >= 0 && b.x0 < npx, x1 = b.x0 + 1 >= 0 && b.x0 + 1 < npx;
  const bool y0 = b.y0 >= 0 && b.y0 < npy, y1 = b.y0 + 1 >= 0 && b.y0 + 1 < npy;
  const int zero = npx * npy;
  Taps t;
  t.o_nw = (x0 && y0) ? b.y0 * npx + b.x0 : zero;
  t.o_ne = (x1 && y0) ? b.y0 * npx + b.x0 + 1 : zero;
  t.o_sw = (x0 && y1) ? (b.y0 + 1) * npx + b.x0 : zero;
  t.o_se = (x1 && y1) ? (b.y0 + 1) * npx + b.x0 + 1 : zero;
  return t;
}

// rgb / weight / label side of one valid voxel, done by lane `gl` of the group of `G` lanes.
// UNDO: the frame's sample leaves the voxel (a = 1 / new_weight, 0 when the voxel empties; the caller has w0 >= 1).
template <bool UNDO = false>
__device__ __forceinline__ void fuse_scalars(const KVol& v, const KFrame& f, const Cam& cam, uint32_t n, float gx,
                                             float gy, int w0, float a, float b, int gl, int G,
                                             unsigned long long* stats) {
  const bool sum = v.accum == SAF_SUM;
  if (gl < 3) {
    const int pix = nearest_index(gx, gy, cam, f.W);
    Bilin bi;
    int x0ok = 0, x1ok = 0, y0ok = 0, y1ok = 0;
    if (f.rgb_bilinear) {
      bi = bilinear_setup(gx, gy, cam.sfx, cam.sfy);
      x0ok = bi.x0 >= 0 && bi.x0 < f.W;
      x1ok = bi.x0 + 1 >= 0 && bi.x0 + 1 < f.W;
      y0ok = bi.y0 >= 0 && bi.y0 < f.H;
      y1ok = bi.y0 + 1 >= 0 && bi.y0 + 1 < f.H;
    }
    for (int ch = gl; ch < 3; ch += G) {
      float s;
      if (f.rgb_bilinear) {  // clip_seem_fusion.py:793-798
        const float* img = f.rgb + ch;
        const int64_t r0 = (int64_t)bi.y0 * f.W, r1 = r0 + f.W;
        const float nw = (x0ok && y0ok) ? img[(r0 + bi.x0) * 3] : 0.f;
        const float ne = (x1ok && y0ok) ? img[(r0 + bi.x0 + 1) * 3] : 0.f;
        const float sw = (x0ok && y1ok) ? img[(r1 + bi.x0) * 3] : 0.f;
        const float se = (x1ok && y1ok) ? img[(r1 + bi.x0 + 1) * 3] : 0.f;
        s = lerp_taps(nw, ne, sw, se, bi);
      } else {  // clipfusion.py:701-706
        s = pix >= 0 ? f.rgb[(int64_t)pix * 3 + ch] : 0.f;
      }
      float* dst = v.rgb + (int64_t)n * 3 + ch;
      *dst = UNDO ? unblend(s, *dst, a, b) : blend(s, *dst, a, b, sum);
    }
    if (gl == 0) {
      v.weight[n] = UNDO ? w0 - 1 : w0 + 1;  // clipfusion.py:715, :721
      if (v.labels && f.label_map) {
        // labels = grid_sample(pano_seg.float(), nearest); one_hot(labels.long())  clip_seem_fusion.py:786-822
        const float lf = pix >= 0 ? f.label_map[pix] : 0.f;
        const long long l = (long long)lf;
        if (l >= 0 && l < v.n_classes) {
          int* c = v.labels + (int64_t)n * v.n_classes + l;
          if (!UNDO)
            *c = *c + 1;
          else if (*c > 0)  // (a count never goes below 0)
            *c = *c - 1;
        } else if (stats && !UNDO) {
          atomicAdd(&stats[3], 1ull);
        }
      }
    }
  }
}

// rgb / weight / label side of one valid voxel handled entirely by ONE lane (the lane-parallel
// part of fuse_rows_kernel): the three channel loads are issued together, then blended and stored.
// The frame's rgb sample for one valid voxel (nearest in ClipFusion, bilinear in ClipSeemFusion); returns the
// nearest pixel index (-1 outside), which the label lookup shares.
__device__ __forceinline__ int sample_rgb_lane(const KFrame& f, const Cam& cam, float gx, float gy, float& s0, float& s1,
                                               float& s2) {
  const int pix = nearest_index(gx, gy, cam, f.W);
  if (f.rgb_bilinear) {  // clip_seem_fusion.py:793-798
    const Bilin bi = bilinear_setup(gx, gy, cam.sfx, cam.sfy);
    const bool x0ok = bi.x0 >= 0 && bi.x0 < f.W, x1ok = bi.x0 + 1 >= 0 && bi.x0 + 1 < f.W;
    const bool y0ok = bi.y0 >= 0 && bi.y0 < f.H, y1ok = bi.y0 + 1 >= 0 && bi.y0 + 1 < f.H;
    const int64_t r0 = (int64_t)bi.y0 * f.W, r1 = r0 + f.W;
    const float* pnw = f.rgb + ((x0ok && y0ok) ? (r0 + bi.x0) * 3 : 0);
    const float* pne = f.rgb + ((x1ok && y0ok) ? (r0 + bi.x0 + 1) * 3 : 0);
    const float* psw = f.rgb + ((x0ok && y1ok) ? (r1 + bi.x0) * 3 : 0);
    const float* pse = f.rgb + ((x1ok && y1ok) ? (r1 + bi.x0 + 1) * 3 : 0);
    const float mnw = (x0ok && y0ok) ? 1.f : 0.f, mne = (x1ok && y0ok) ? 1.f : 0.f;
    const float msw = (x0ok && y1ok) ? 1.f : 0.f, mse = (x1ok && y1ok) ? 1.f : 0.f;
    // out-of-image taps: value forced to +0 (x * 0 would keep NaN/inf of pixel 0 alive)
    float nw[3], ne[3], sw[3], se[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      nw[ch] = pnw[ch]; ne[ch] = pne[ch]; sw[ch] = psw[ch]; se[ch] = pse[ch];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      nw[ch] = mnw != 0.f ? nw[ch] : 0.f; ne[ch] = mne != 0.f ? ne[ch] : 0.f;
      sw[ch] = msw != 0.f ? sw[ch] : 0.f; se[ch] = mse != 0.f ? se[ch] : 0.f;
    }
    s0 = lerp_taps(nw[0], ne[0], sw[0], se[0], bi);
    s1 = lerp_taps(nw[1], ne[1], sw[1], se[1], bi);
    s2 = lerp_taps(nw[2], ne[2], sw[2], se[2], bi);
  } else {  // clipfusion.py:701-706
    const float* px = f.rgb + (int64_t)(pix >= 0 ? pix : 0) * 3;
    const float t0 = px[0], t1 = px[1], t2 = px[2];
    s0 = pix >= 0 ? t0 : 0.f;
    s1 = pix >= 0 ? t1 : 0.f;
    s2 = pix >= 0 ? t2 : 0.f;
  }
  return pix;
}
// labels = grid_sample(pano_seg.float(), nearest); one_hot(labels.long())          clip_seem_fusion.py:786-822
// ATOMIC: several hits of one voxel may be counted by different lanes at the same time (integer adds commute).
// UNDO (never with ATOMIC): the frame's vote is taken back -- a count never goes below 0, a label that was dropped forward is skipped.
template <bool ATOMIC, bool UNDO = false>
__device__ __forceinline__ void count_label_lane(const KVol& v, const KFrame& f, uint32_t n, int pix,
                                                 unsigned long long* stats) {
  if (v.labels && f.label_map) {
    const float lraw = f.label_map[pix >= 0 ? pix : 0];
    const float lf = pix >= 0 ? lraw : 0.f;
    const long long l = (long long)lf;
    if (l >= 0 && l < v.n_classes) {
      int* c = v.labels + (int64_t)n * v.n_classes + l;
      if (UNDO) {
        if (*c > 0) *c = *c - 1;
      } else if (ATOMIC) {
        atomicAdd(c, 1);
      } else {
        *c = *c + 1;
      }
    } else if (stats && !UNDO) {
      atomicAdd(&stats[3], 1ull);
    }
  }
}
template <bool UNDO = false>
__device__ __forceinline__ void fuse_scalars_lane(const KVol& v, const KFrame& f, const Cam& cam, uint32_t n,
                                                  float gx, float gy, int w0, float a, float b,
                                                  unsigned long long* stats) {
  const bool sum = v.accum == SAF_SUM;
  float s0, s1, s2;
  const int pix = sample_rgb_lane(f, cam, gx, gy, s0, s1, s2);
  float* dst = v.rgb + (int64_t)n * 3;
  const float o0 = dst[0], o1 = dst[1], o2 = dst[2];
  dst[0] = UNDO ? unblend(s0, o0, a, b) : blend(s0, o0, a, b, sum);
  dst[1] = UNDO ? unblend(s1, o1, a, b) : blend(s1, o1, a, b, sum);
  dst[2] = UNDO ? unblend(s2, o2, a, b) : blend(s2, o2, a, b, sum);
  v.weight[n] = UNDO ? w0 - 1 : w0 + 1;  // clipfusion.py:715, :721
  count_label_lane<false, UNDO>(v, f, n, pix, stats);
}

int make_kframe(const saf_frame* fr, KFrame* kf) {
  if (!fr) return fail(SAF_E_INVALID, "frame is NULL");
  if (fr->height <= 0 || fr->width <= 0 || fr->npy <= 0 || fr->npx <= 0)
    return fail(SAF_E_INVALID, "bad frame shape %dx%d map %dx%d", fr->height, fr->width, fr->npy, fr->npx);
  if ((int64_t)fr->height * fr->width >= (1ll << 30)) return fail(SAF_E_UNSUPPORTED, "image too large");
  if (!fr->depth || !fr->rgb || !fr->pose || !fr->K || !fr->feat_map) return fail(SAF_E_INVALID, "frame has a NULL buffer");
  kf->H = fr->height; kf->W = fr->width; kf->npy = fr->npy; kf->npx = fr->npx;
  kf->rgb_bilinear = fr->rgb_bilinear;
  kf->depth = fr->depth; kf->rgb = fr->rgb; kf->pose = fr->pose; kf->K = fr->K;
  kf->label_map = fr->label_map;
  return SAF_OK;
}


struct ScopedPair {
  saf_profiler* p;
  hipStream_t s;
  int idx;
  ScopedPair(saf_profiler* prof, int cls, int64_t frame_no, hipStream_t stream) : p(prof), s(stream), idx(-1) {
    if (p && p->used < p->capacity && frame_no % p->stride == 0) {
      idx = p->used++;
      p->pairs[idx].cls = cls;
      (void)hipEventRecord(p->pairs[idx].a, s);
    }
  }
  ~ScopedPair() {
    if (idx >= 0) (void)hipEventRecord(p->pairs[idx].b, s);
  }
};

}  // namespace

// the windowed path (saf_window.hip), called by saf_fuse_frames
size_t window_workspace_bytes(int64_t n_vox, int D, int P, bool bricks, int H = 0, int W = 0, bool labels = false);
// ---- The route of a fusion call: the ONE statement of which path takes it (fuse_route, saf_window.hip).  saf_fuse_path,
// saf_fuse_session_ok, the session entries, fuse_many, win_plan and the three saf_fuse_workspace_bytes* entries ask these
// functions and own no rule of their own.
enum FusePath {
  kPathPerFrame = 0,  // the per-frame pipeline (saf_fuse.hip)
  kPathRows,          // windowed: the frame-ordered row kernel (bit-identical to fusing frame after frame)
  kPathSums,          // windowed: the order-free row kernel (a row's samples of the window summed in registers, one blend per row)
  kPathBricks,        // windowed: the brick form (saf_brick.hip)
};
struct FuseRoute {
  FusePath path;  // what saf_fuse_frames (and _recycled, _slabs) does with the call
  bool session;   // a streaming session takes these frames (saf_fuse_session_ok)
};
FuseRoute fuse_route(const KVol& kv, const saf_frame* frames, int32_t n_frames, size_t workspace_bytes, const Knobs& kn);
// The two width rules.  The row kernels move whole 1 KiB pieces of a row per wave instruction: feat_dim a multiple of 256 up to
// 1024 -- of 512 for 16-bit rows (bf16 and fp16), where a lane moves 8 channels.  The brick form: brick_form_takes (saf_window_dev.h).
inline bool row_kernel_takes(int D, bool rows16) { return D % 256 == 0 && D <= 1024 && (!rows16 || D % 512 == 0); }
// Whether a call on such a volume asks for the brick form (it gets it where the workspace has room for its pools): the default
// for the widths the row kernel does not take, what SAF_WIN_FORM=bricks asks for, never under SAF_WIN_FORM=rows.
bool brick_form_applies(const KVol& kv, const Knobs& kn);
// ... and whether a workspace sized WITHOUT the volume (saf_fuse_workspace_bytes: a width, no dtype, no grid) holds the pools
bool brick_form_sized_for(int D, const Knobs& kn);
// Streams / events for running the classification of window w + 1 beside the row kernel of window w (may be NULL:
// everything on the caller's stream).
struct WinOverlap {
  hipStream_t aux;
  hipEvent_t fork, join, cls_done[2], fuse_done[2];
  hipEvent_t tiles;  // (may be NULL) the later windows' depth tiles, computed on the caller's stream ahead of their classification
};
// saf_fuse_frames_slabs: every frame into x-planes [x0[k], x0[k] + nx[k]) for k = 0 .. n - 1 in turn; done[k] (may be NULL):
// a hipEvent_t recorded on the caller's stream behind slab k's last row kernel.
struct WinSlabs {
  int n;
  const int32_t *x0, *nx;
  void* const* done;
};
// A streaming session (saf_fuse_session_*; saf_window.hip): the open window's state between two pushes.
struct WinStream {
  bool open = false;        // a window is open: `filled` of its frames are classified, its row kernel is not launched
  int filled = 0;
  int n_windows = 0;        // windows closed so far (parity of headers / mask planes, tile slots, "first window")
  bool have_shape = false;  // kv / kf0 are those of the session's frames
  KVol kv;
  KFrame kf0;
  long long pushed = 0;     // frames classified so far in this session
  long long prepared = 0;   // frames whose depth tiles are computed (stream_prepare runs ahead of stream_push: >= pushed, or behind it when unused)
};
int stream_prepare(const KVol& kv, const saf_frame* frames, int32_t n_frames, void* workspace, size_t workspace_bytes, hipStream_t ts,
                   const Knobs& kn, WinStream* st);
int stream_push(const KVol& kv, const saf_frame* frames, int32_t n_frames, void* workspace, size_t workspace_bytes, uint64_t* stats,
                hipStream_t s, hipEvent_t ready, hipStream_t tile_stream, const WinOverlap* ov, const Knobs& kn, WinStream* st);
int stream_close(void* workspace, size_t workspace_bytes, uint64_t* stats, hipStream_t s, const WinOverlap* ov, const Knobs& kn, WinStream* st,
                 bool preopen);
// recycled: the volume's feature rows were not cleared when its scalars were (saf_fuse_frames_recycled) -- the rows of voxels
// whose weight is still 0 when the call is over are zeroed by it, beside the last window's row kernel where the schedule allows.
int fuse_many_windowed(const KVol& kv, const saf_frame* frames, int32_t n_frames, void* workspace, size_t workspace_bytes,
                       uint64_t* stats, saf_profiler* prof, hipStream_t s, const WinOverlap* ov, const Knobs& kn,
                       const WinSlabs* slabs = nullptr, bool recycled = false, bool undo = false);
// undo (saf_unfuse_frames_windowed): the same schedule with the backward classification and row kernel -- the frames leave the
// volume window by window; only where unfuse_windowed says so (f32 running means, the order-free form).  (saf_window.hip)
bool unfuse_windowed(const KVol& kv, const saf_frame* frames, int32_t n_frames, size_t workspace_bytes, const Knobs& kn);
// saf_misc.hip (clear_rows): zero the feature rows of the voxels n in [0, kv.N) with weight[n] == 0 and -- masks may be NULL -- no
// bit set in masks[p * mask_plane + n] for p < n_planes (the hit masks of a window whose row kernel may be running: it writes exactly
// the rows with a bit set, this kernel only the others).
int clear_rows(void* feat, const int* weight, int64_t first, int64_t n_rows, int esz, int row_bytes, const uint32_t* masks,
               size_t mask_plane, int n_planes, const Knobs& kn, hipStream_t s);
inline int launch_clear_unwritten(const KVol& kv, const uint32_t* masks, size_t mask_plane, int n_planes, const Knobs& kn, hipStream_t s) {
  const int esz = kv.e16 ? 2 : 4;
  return clear_rows(kv.feat, kv.weight, 0, (int64_t)kv.N, esz, kv.D * esz, masks, mask_plane, n_planes, kn, s);
}
KVol slab_kvol(const KVol& kv, int x0, int nx);
// slab k of a call's slab list lies inside the volume
inline int check_slab(const KVol& kv, const WinSlabs& sl, int k) {
  if (sl.x0[k] < 0 || sl.nx[k] <= 0 || sl.x0[k] + sl.nx[k] > kv.nx) return fail(SAF_E_INVALID, "slab %d outside the volume", k);
  return SAF_OK;
}

}  // namespace saf
