/*
 * saf.h -- C ABI of the MI355X-native fusion hot path ("saf" = spatially-aware fusion).
 *
 * The reference (cy-xu/spatially_aware_AI) has no FFI layer: its boundary for this path is the
 * Python class API.  This header is the drop-in boundary *underneath* that API:
 * plain pointers and sizes, no torch types.  Every entry point names the reference code it
 * replaces.  The Python host classes in spatially_aware_ai_amd/ bind these through ctypes
 * (see INTEGRATION.md for the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - all data pointers are DEVICE pointers (HIP, gfx950) unless a parameter says "host";
 *   - nothing here owns volume memory: the caller (torch) allocates and keeps it alive;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and re-entrant.  Process-wide state is limited to: the thread-local error string, a
 *     per-device pool of the auxiliary stream / events of the per-frame pipeline, and a per-device
 *     asynchronous error latch (saf_poll_async_error);
 *   - return value: 0 = ok, <0 = error (SAF_E_*), text via saf_last_error();
 *   - voxel flat index n = (x*ny + y)*nz + z, the C-order flattening of meshgrid(ij)
 *     (clipfusion.py:617-622); 64-bit offsets are used wherever n*D can exceed 2^31.
 *
 * oracle/saf_oracle.c implements CPU twins (saf_oracle_*) of the compute entry points with the
 * same structs and HOST pointers; they are test infrastructure only.
 */
#ifndef SAF_H
#define SAF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAF_ABI_VERSION 7

enum saf_status {
  SAF_OK = 0,
  SAF_E_INVALID = -1,   /* bad argument (NULL pointer, non-positive size, misaligned buffer) */
  SAF_E_WORKSPACE = -2, /* workspace too small */
  SAF_E_HIP = -3,       /* HIP runtime error (launch failure, ...) */
  SAF_E_UNSUPPORTED = -4
};

enum saf_dtype { SAF_F32 = 0, SAF_BF16 = 1, SAF_F16 = 2 };

/* How per-voxel features are folded in (clipfusion.py:715-721). */
enum saf_accum_mode {
  SAF_RUNNING_MEAN = 0, /* reference semantics: x <- s*(1/w') + x*(w*(1/w')) in that op order */
  SAF_SUM = 1           /* x <- x + s ; used by the frame-sharded multi-GPU path, finalised by
                           saf_merge_finalize after the RCCL reduction */
};

/*
 * The dense fusion volume: the registered buffers of ClipFusion (clipfusion.py:605-625) and
 * ClipSeemFusion (clip_seem_fusion.py:640-672).  `xyz_world` is replaced by three per-axis
 * coordinate tables (xyz_world[n] = (axis_x[x], axis_y[y], axis_z[z]) for any elementwise
 * construction from meshgrid(ij)), so the sweep never reads the 12*N-byte buffer.
 */
typedef struct saf_volume {
  int32_t nx, ny, nz;
  int32_t feat_dim;       /* D = n_clip_feats */
  int32_t n_classes;      /* width of labels_one_hot (143) or 0 when there is no label histogram */
  int32_t feat_dtype;     /* saf_dtype of clip_feat; SAF_F32 is the reference layout.  SAF_BF16 and SAF_F16 (feat_dim a multiple of 8,
                             16-byte aligned rows): widened exactly, blended in fp32, narrowed with ONE round-to-nearest-even per
                             update -- what torch.Tensor.to(dtype) does (fp16: subnormals kept, +-inf beyond +-65504).  SAF_F16 is the
                             dtype saf_query_scan_wide reads in place; it takes SAF_RUNNING_MEAN only (SAF_SUM: SAF_E_UNSUPPORTED --
                             sums over many frames leave fp16's range, and saf_merge_finalize is fp32-only) */
  int32_t accum_mode;     /* saf_accum_mode */
  float trunc;            /* truncation distance in metres (self.trunc) */
  const float* axis_x;    /* [nx] */
  const float* axis_y;    /* [ny] */
  const float* axis_z;    /* [nz] */
  float* tsdf;            /* [N]       f32 */
  int32_t* tsdf_weight;   /* [N]       i32 */
  int32_t* weight;        /* [N]       i32 */
  float* rgb;             /* [N,3]     f32 */
  void* clip_feat;        /* [N,D]     feat_dtype */
  int32_t* labels_one_hot;/* [N,n_classes] i32 or NULL */
} saf_volume;

/*
 * One posed RGB-D frame plus the backbone outputs that integrate() consumes
 * (clipfusion.py:627-645, clip_seem_fusion.py:676-695, :755-760).
 */
typedef struct saf_frame {
  int32_t height, width;
  const float* depth;     /* [H,W]   metres; 0 = missing */
  const float* rgb;       /* [H,W,3] 0..1, channel-last exactly as the loaders yield it */
  const float* pose;      /* [4,4]   camera->world, row-major (device memory) */
  const float* K;         /* [3,3]   intrinsics, row-major (device memory) */
  const float* feat_map;  /* [Dm,npy,npx] f32, Dm >= D: Clip.img_inference_tiled output for this frame;
                             only the first D channels are used (clipfusion.py:709) */
  int32_t npy, npx;
  const float* label_map; /* [H,W] f32 class ids = pano_seg.float() (clip_seem_fusion.py:760) or NULL */
  int32_t rgb_bilinear;   /* 0: nearest (clipfusion.py:701-706); 1: bilinear (clip_seem_fusion.py:793-798) */
} saf_frame;

/* Counters the fuse kernels add to (device memory, SAF_STATS_WORDS x u64 -- 16 since ABI version 3, 8 before --, caller zeroes
 * them when it wants):
 *  [0] sum of Nv (valid voxels)  [1] sum of Nt (tsdf-valid voxels)  [2] frames fused
 *  [3] labels outside [0,n_classes) that were dropped (the reference raises instead)
 *  [4] fuse workgroups that gave up waiting for their frame's sweep (must stay 0)
 *  [5] feature rows read-modify-written by window kernels (= sum over windows of |union of valid sets|;
 *      0 when the per-frame pipeline ran)  [6] voxels whose TSDF a window's classification updated
 *      (sum over windows of |union of tsdf-valid sets|)  [7] disagreements between the classification's guarded pixel path and
 *      the reference's chain, counted only with SAF_CLS_VERIFY=1 in the environment (a self-check; must stay 0)
 *  [8..12] the windowed path's frame cull (a wave tests its 4 x 4 x 16-voxel brick against the 32 frames of a classification
 *      launch before it classifies any voxel; clipfusion.py:647-679 has no counterpart -- it projects every voxel into every
 *      frame): [8] (brick, frame) pairs tested, and of those dropped because the brick lies [9] behind the camera, [10]
 *      farther than the frame's largest depth + trunc, [11] outside the view frustum, [12] more than trunc behind the largest
 *      depth of the pixels it projects onto (occluded).  A dropped pair has no valid and no tsdf-valid voxel; tests assert that
 *      every reason fires on the cameras they fuzz.
 *  [13] [14] saf_unfuse_frames only (forward fusion leaves them 0): updates it skipped because the voxel's count was already 0 --
 *      [13] on the weight side (valid voxels: weight, rgb, feature row, label count), [14] on the tsdf_weight side (tsdf-valid
 *      voxels).  Non-zero means a frame was taken out that was never fused, or was fused under another pose.
 *  [15] reserved (0). */
#define SAF_STATS_WORDS 16
/* frames per window of the windowed path of saf_fuse_frames (stats[5] and [6] count per window); SAF_WIN_FRAMES=64 in the
 * environment selects 64-frame windows */
#define SAF_WINDOW_FRAMES 128

const char* saf_last_error(void);
int saf_abi_version(void);

/* Bytes of device scratch saf_fuse_frame(s) needs for a volume of n_voxels and a feature map of
 * feat_dim x npy x npx (compact list of valid voxels + re-laid-out feature map + counters). */
size_t saf_fuse_workspace_bytes(int64_t n_voxels, int32_t feat_dim, int32_t npy, int32_t npx);
/* The same for ONE volume (its grid, width and feature dtype are known): the brick form's segment pools -- 6.5 GB at
 * 256^3 -- are reserved only when that form would run for it (feat_dim a multiple of 64 that the row kernel does not
 * take, or SAF_WIN_FORM=bricks); the default 512-channel f32 / bf16 volumes end at 0.55 GB.  0 for a bad descriptor.
 * An SAF_F16 volume gets what an SAF_BF16 volume gets where the row kernel takes it (feat_dim 512, 1024); at every other width
 * and under SAF_WIN_FORM=bricks it gets LESS: the brick form does not take fp16, so its pools are never reserved (this entry and
 * saf_fuse_workspace_bytes_for_frames). */
size_t saf_fuse_workspace_bytes_for(const saf_volume* vol, int32_t npy, int32_t npx);
/* The same, with room for the frames' depth images (height x width) re-laid-out in 4 x 8-pixel tiles, four windows of 128
 * frames of them (0.63 GB at 640 x 480): with such a workspace the windowed path's classification gathers depth from the
 * tiled copies -- half the cache lines per brick and frame --, with a smaller one from the frames'
 * own row-major images; results are identical either way.  New in round 5; nothing to mirror in the reference.
 * Round 6: for a volume that counts labels (ClipSeemFusion) it also holds ONE window of the frames' rgb and label images packed as
 * {r, g, b, label} pixels in 4 x 2-pixel tiles (0.63 GB at 640 x 480): the row kernel then takes a hit's bilinear colour and its
 * class from four 16-byte gathers instead of thirteen 4-byte ones (clip_seem_fusion.py:786-798); identical results either way. */
size_t saf_fuse_workspace_bytes_for_frames(const saf_volume* vol, int32_t npy, int32_t npx, int32_t height, int32_t width);

/*
 * Fuse ONE frame into the volume: replaces the body of ClipFusion.integrate after the CLIP call
 * (clipfusion.py:647-721) / ClipSeemFusion.integrate (clip_seem_fusion.py:697-822) for batch
 * element i: projection + depth test (a2), TSDF running mean (a3), valid-voxel compaction (a4),
 * feature / rgb / label gather (a5), running-mean fuse (a6), label histogram (a7).
 * `stats` may be NULL.
 */
int saf_fuse_frame(const saf_volume* vol, const saf_frame* frame, void* workspace,
                   size_t workspace_bytes, uint64_t* stats, void* stream);

/* The same for n_frames frames in order (host array of descriptors); one host call, no host
 * synchronisation between frames -- the loop of clipfusion.py:1125-1133.
 * Two device paths.  Which voxels are touched, weights, tsdf, tsdf_weight, rgb and label counts are identical bit for bit
 * on both; so are the feature rows with SAF_WIN_FORM=rows:
 *  - per-frame pipeline: one sweep + one fuse kernel per frame (any shape);
 *  - windowed, voxel-major (16 or more frames of one shape, feat_dim a multiple of 64 up to 8192): per window of
 *    SAF_WINDOW_FRAMES frames one classification launch per 32 frames (projection, depth test, TSDF in registers, one
 *    frame-mask word per voxel; any grid) and one row kernel that reads and writes every touched feature row ONCE per
 *    window.  The row kernel's form (environment SAF_WIN_FORM, read per call):
 *      sums   (default where it applies: f32 volume with feat_dim a multiple of 256, bf16 / fp16 with a multiple of 512, <= 1024) a
 *             row's samples of the window are summed in registers and the row is blended once, (w0 old + sum) / (w0 + k): the
 *             running mean of clipfusion.py:715-721 with the window's k updates folded into one -- feature values within fp32
 *             rounding of frame-after-frame fusion (bf16 / fp16: one rounding per window instead of one per hit), reproducible
 *             bit for bit from run to run.  For a bf16 (fp16) volume this form also keeps the window's feature maps in bf16
 *             (fp16), rounded once, to nearest even, when they are re-laid for the taps: exact when the backbone emitted features
 *             of that type (BASELINE config 3), otherwise one more rounding at the volume's own precision per tap.  An fp16
 *             image has fp16's range: a MAP value beyond +-65504 is +-inf in it, and a row that taps it stores NaN (inf x a tap
 *             weight of 0) where the rows form and the per-frame pipeline store +-inf;
 *             SAF_WIN_MAPS16=0 keeps fp32 maps and takes the rows form, SAF_WINDOW_BF16=0 the per-frame pipeline (both: bf16
 *             and fp16 volumes alike);
 *      rows   the same widths, hits applied one by one in frame order: feature rows bit-identical to the per-frame pipeline;
 *      bricks every other width (and on request): brick-resident rows, map taps shared, fixed-point sums; same contract as sums.
 *             f32 and bf16 volumes only: an fp16 volume's other widths stay on the per-frame pipeline (saf_fuse_path: 0), and
 *             SAF_WIN_FORM=bricks on an fp16 volume of a width the row kernel takes gets the default form (sums).
 *    SAF_WINDOW=0 in the environment forces the per-frame pipeline. */
int saf_fuse_frames(const saf_volume* vol, const saf_frame* frames, int32_t n_frames,
                    void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);

/* Take n_frames fused frames OUT of the volume again, in the order given (new capability: the de-integration step of a map
 * that follows pose corrections; clipfusion.py has no counterpart -- its running means, :715-721 and clip_seem_fusion.py:736-744,
 * :808-822, only ever grow).  Same descriptors and workspace as saf_fuse_frames; always the per-frame pipeline run backwards (one
 * sweep + one row kernel per frame), whatever saf_fuse_path says forward, at every width and grid that pipeline takes.
 * Which voxels a frame touches depends on the frame (depth, pose, K) and the grid only, never on the volume's state: the valid /
 * tsdf-valid sets and the samples (clamped sdf, rgb, feature taps, label) are computed by the forward kernels' own code, so a
 * frame leaves exactly the voxels it entered.  Per touched voxel with count w (weight, resp. tsdf_weight) before, w' = w - 1 after:
 *   w' >= 1   x' = x * b - s * r   with  r = 1 / (float)w',  b = (float)w * r   -- in this order: r by IEEE division, b one rounded
 *             product, x * b and s * r rounded separately, then one rounded difference (no FMA).  The TSDF takes r from the
 *             hardware reciprocal (1 ulp), as the forward sweep does.  One removal adds about five roundings of the size of the
 *             values involved, and an error already in the mean of w samples grows to w / (w - 1) of itself.
 *   w' == 0   the voxel returns to its constructed state: exact zeros for the TSDF value, rgb and the whole feature row (never
 *             x - s).  A volume with every frame taken out again is bit for bit a fresh one, and "a weight-0 voxel has a zero
 *             row" holds without a clear pass.
 *   w  == 0   guard: the update is skipped, nothing of the voxel is written, stats[13] (weight side) / stats[14] (tsdf_weight
 *             side) count it.  Counts never go negative.
 *   labels    minus one in the class the frame votes for, unless that count is already 0 (skipped, not counted); a label outside
 *             [0, n_classes) was dropped forward (stats[3]) and is skipped here.
 * stats[0..3] are not touched.  SAF_E_UNSUPPORTED, before anything is launched, for feat_dtype SAF_BF16 / SAF_F16 (a stored
 * 16-bit mean carries 2^-9 / 2^-12 relative rounding, which a removal multiplies by about w) and for accum_mode SAF_SUM (sums
 * belong to the multi-rank job).  A volume that saf_fuse_frames_recycled would take (rows of weight-0 voxels not yet cleared)
 * must be cleared first (saf_clear_unwritten_rows): the guard never reads such rows, but w' == 0 relies on nothing else holding
 * them. */
int saf_unfuse_frames(const saf_volume* vol, const saf_frame* frames, int32_t n_frames,
                      void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);
int saf_unfuse_frame(const saf_volume* vol, const saf_frame* frame, void* workspace,
                     size_t workspace_bytes, uint64_t* stats, void* stream);

/* The windowed removal (added under ABI 7): the same frames leave the same voxels, a window at a time -- per window of
 * SAF_WINDOW_FRAMES frames (64 under SAF_WIN_FRAMES=64) one backward classification launch per 32 frames (the TSDF leaves in
 * registers, frame after frame) and one backward row kernel that reads and writes every touched feature row ONCE, where
 * saf_unfuse_frames reads and writes it once per frame.  A bulk call: no streaming-session form.
 *   saf_unfuse_path             1 if saf_unfuse_frames_windowed takes the call: an SAF_F32, SAF_RUNNING_MEAN volume with feat_dim
 *                               256 / 512 / 768 / 1024, 16 or more frames of one shape, a workspace the windowed forward path
 *                               accepts, SAF_WINDOW not 0 and SAF_WIN_FORM unset or "sums" (only the order-free form is built
 *                               backwards); 0 if only saf_unfuse_frames takes it; -1 for bad arguments.  Host-only, launches nothing.
 *   saf_unfuse_frames_windowed  signature, refusals and counters of saf_unfuse_frames; SAF_E_UNSUPPORTED before anything is
 *                               launched wherever saf_unfuse_path is not 1.
 * Arithmetic, per touched voxel:
 *   TSDF     frame by frame in frame order, tw the voxel's tsdf_weight and t the frame's clamped sdf: tw == 0 -> skipped,
 *            nothing written, stats[14]; tw - 1 == 0 -> 0.0f exactly; else r = rcp((float)(tw - 1)) (hardware reciprocal),
 *            b = (float)tw * r, tsdf = tsdf * b - t * r (two products rounded separately, no FMA) -- saf_unfuse_frames' order.
 *   weight   w0 before, k hits in the window: k_eff = min(k, w0).  The FIRST k_eff hits in frame order are removed, the other
 *            k - k_eff found the voxel empty and are counted in stats[13]; weight' = w0 - k_eff.  (What frame-after-frame
 *            removal does: a weight only falls during a removal.)
 *   rgb      the first k_eff hits one by one in frame order with saf_unfuse_frames' x * b - s * r; exact zeros at weight' == 0.
 *   labels   minus one per removed hit in its class, never below 0; a class outside [0, n_classes) is skipped.
 *   feature row   w0 == 0: nothing of the voxel is read or written.  k >= w0 > 0: an exact zero row is stored.  k < w0: the
 *            accumulator starts as the old row; every hit adds its four taps by four chained FMAs, in frame order, with tap weights
 *            scaled (one rounding each) by -(1 / (float)w0); the row leaves as acc * ((float)w0 * (1 / (float)(w0 - k))).
 * tsdf, tsdf_weight, weight, rgb, the label histograms and stats[13] / stats[14] are BIT FOR BIT those of saf_unfuse_frames on
 * the same frames in the same order, guard cases included; emptied rows are exact zeros either way.  The other feature rows are
 * within fp32 rounding of it, not equal: |row - (w0 old - S) / (w0 - k)| <= 16 * 2^-24 * k * w0 / (w0 - k) * M per element (S the
 * sum of the k samples, M the largest magnitude among the old row and the samples), reproducible bit for bit from run to run.
 * stats[0..3], [5], [6] and [8..12] are not touched. */
int saf_unfuse_path(const saf_volume* vol, const saf_frame* frames, int32_t n_frames, size_t workspace_bytes);
int saf_unfuse_frames_windowed(const saf_volume* vol, const saf_frame* frames, int32_t n_frames,
                               void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);

/* Copy one frame's inputs (depth, rgb, pose, K, feature map, label map -- all f32) from `src` into the buffers `dst`
 * points to, in ONE launch: the host queue behind integrate() keeps the frames of small calls in a staging ring until a
 * window is full.  The source feature map is addressed through element strides (Clip.img_inference_tiled returns a
 * permuted view); feat_channels = channels to copy; everything else is contiguous.  src->feat_map may be NULL (the queue
 * computes the feature maps later, in one backbone batch per flush): nothing is copied for it.  depth, rgb and label_map may be
 * NULL in BOTH `src` and `dst`: images the caller lends the queue where they lie (the frame descriptors of the later fuse call
 * point at them) instead of having them copied. */
int saf_stage_frame(const saf_frame* src, int32_t feat_channels, int64_t feat_stride_c, int64_t feat_stride_y,
                    int64_t feat_stride_x, const saf_frame* dst, void* stream);

/* Which device path saf_fuse_frames would take for this call: 1 = windowed (never reads the feature rows of voxels
 * with weight 0), 0 = per-frame pipeline, -1 = invalid arguments.  Host-only, launches nothing. */
int saf_fuse_path(const saf_volume* vol, const saf_frame* frames, int32_t n_frames, size_t workspace_bytes);

/*
 * Streaming session (new in ABI version 3): the loop of clip_seem_fusion.py:303-313 / clipfusion.py:1125-1133 hands over ONE
 * frame per integrate() call; the host queue behind it (spatially_aware_ai_amd/clipfusion.py) stages the frames and pushes them
 * 32 at a time.  A separate saf_fuse_frames call per window exposes the window's whole classification (nothing of the call runs
 * beside it: 3.7 ms at 256^3) and cannot start before the window's last frame has arrived; a session keeps ONE pipeline:
 *   saf_fuse_session_ok      1 if a session takes these frames for this volume and workspace (what the windowed ROW forms take, on
 *                            two streams: SAF_WIN_OVERLAP != 0, in windows of SAF_WINDOW_FRAMES frames: SAF_WIN_FRAMES unset), 0 if
 *                            not (use saf_fuse_frames), -1 for bad arguments.
 *   saf_fuse_session_push    classifies the frames at once -- one launch (one mask plane of the open window) per 32 frames, on the
 *                            session's classification stream -- and, when a window (SAF_WINDOW_FRAMES) is complete, launches its row
 *                            kernel on `stream`: the launches of the following pushes run beside it.  Every push but a window's last
 *                            brings a multiple of 32 frames.  Same volume, workspace, counters and frame shapes until finish.
 *                            The frames' device buffers stay untouched until the stream has passed their window's row kernel.
 *                            `ready_event` (a hipEvent_t, may be NULL): recorded by the caller behind whatever produces these
 *                            frames (their staging), on any stream, and behind the previous finish of this session; the
 *                            classification waits for it INSTEAD of for everything queued on `stream` -- where the previous
 *                            window's row kernel sits, the kernel it is meant to run beside.  NULL: it waits for `stream`.
 *                            `tile_stream` (a hipStream_t, may be NULL): the stream the frames were staged on (the one `ready_event`
 *                            was recorded on: with it the event itself is not waited for); the launches' depth tile maxima (two
 *                            small kernels per 32 frames) run there, behind the staging, instead of in the classification chain.  That stream must be ordered behind the row kernel of the window four windows back (the
 *                            tile region holds four windows; with windows of SAF_WINDOW_FRAMES frames the host queue's staging
 *                            ring of 4 x SAF_WINDOW_FRAMES slots has the same period.  With SAF_WIN_FRAMES=64 it has not -- the
 *                            region turns over twice per turn of the ring -- and a session refuses: saf_fuse_session_ok is 0,
 *                            push and prepare return SAF_E_UNSUPPORTED, and saf_fuse_frames cuts the shorter windows itself).
 *   saf_fuse_session_prepare (optional) the depth tile maxima of frames that will be pushed NEXT, in order, computed on `stream` (the one
 *                            they were staged on) a call ahead of their push: a `ready_event` recorded behind it has completed by the
 *                            time the frames are pushed, and the push then queues its launch with no cross-stream wait in front.
 *   saf_fuse_session_finish  launches the row kernel of the window that is still open; behind it (in stream order) the volume
 *                            holds every pushed frame, bit for bit as one saf_fuse_frames call over them leaves it.
 *   saf_fuse_session_abandon drops the open window without fusing its rows (the volume is being reset: its classification has
 *                            updated the TSDF, or is still doing so).  Launches no kernel; `stream` (ABI version 7; any stream)
 *                            waits for the session's classification stream, so that what the caller queues behind `stream` --
 *                            zeroing the volume -- comes after the last store of the abandoned frames.
 *   saf_fuse_session_pending frames of the open window (0: none).
 * `stream`: the same stream for every call of a session (one of the host queue's own, so that the caller's stream can stage
 * later frames meanwhile).  Not thread-safe per session; sessions are independent of each other.
 */
typedef struct saf_fuse_session saf_fuse_session;
saf_fuse_session* saf_fuse_session_create(void);
int saf_fuse_session_ok(const saf_volume* vol, const saf_frame* frames, int32_t n_frames, size_t workspace_bytes);
int saf_fuse_session_push(saf_fuse_session* session, const saf_volume* vol, const saf_frame* frames, int32_t n_frames,
                          void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream, void* ready_event,
                          void* tile_stream);
int saf_fuse_session_prepare(saf_fuse_session* session, const saf_volume* vol, const saf_frame* frames, int32_t n_frames,
                             void* workspace, size_t workspace_bytes, void* stream);
int saf_fuse_session_finish(saf_fuse_session* session, void* stream);
int saf_fuse_session_abandon(saf_fuse_session* session, void* stream);
int saf_fuse_session_pending(const saf_fuse_session* session);
void saf_fuse_session_destroy(saf_fuse_session* session);

/*
 * The 7 x 7 depthwise convolution of a ConvNeXt block, channels-last (backbone op of BASELINE config 3's panoptic encoder:
 * kMaX-DeepLab's ConvNeXt-L behind KmaxSegmentationModel.run_on_image, handy_utils.py:29-161; in PyTorch
 * nn.Conv2d(C, C, 7, padding=3, groups=C)).  MIOpen runs these through naive_conv; the op is tiny and L2 bound.
 *   x, y    [batch, H, W, C] of `dtype` (SAF_F32 / SAF_BF16 / SAF_F16), C contiguous and a multiple of 8, 16-byte aligned
 *   w_kkc   [7, 7, C] f32: PyTorch's weight [C, 1, 7, 7] permuted once by the host
 *   bias    [C] f32 or NULL
 * fp32 accumulation, one rounding to `dtype` on the way out; zero padding of 3 pixels.
 */
int saf_dwconv7x7_nhwc(const void* x, const float* w_kkc, const float* bias, void* y, int32_t batch, int32_t height,
                       int32_t width, int32_t channels, int32_t dtype, void* stream);

/* Zero the clip_feat rows of voxels [first, first + n) whose weight is 0.  A volume recycled for a new scan may skip the
 * up-front clear of its 4*D*N feature bytes: zero `weight` (and the other small buffers), fuse through the windowed path
 * only, and call this before anything else reads clip_feat (the Python host does all of that behind reset()). */
int saf_clear_unwritten_rows(const saf_volume* vol, int64_t first_voxel, int64_t n_voxels, void* stream);

/* The per-frame pipeline hands sweep(i) to fuse(i) on the device; a fuse workgroup that waited ~2 s without
 * seeing its sweep gives up (stats[4]) and sets a host-visible latch.  The NEXT saf_fuse_frame(s) call on that
 * device -- or this poll, which launches nothing -- returns SAF_E_HIP once (the volume of the earlier call is
 * incomplete; its stats[4] says so for as long as the volume lives) and clears the latch: a stall that has passed
 * does not disable fusion for the rest of the process. */
int saf_poll_async_error(void);

/*
 * Optional per-kernel timing: a pool of HIP event pairs recorded on the launch stream around each
 * kernel of saf_fuse_frames_profiled (class 0 = prep, 1 = sweep / window classification, 2 = fuse /
 * window row kernel).  Recording is
 * asynchronous; saf_profiler_read must be called after the stream has been synchronised.
 * Used by bench.py for the roofline line; the product path passes NULL.
 */
typedef struct saf_profiler saf_profiler;
saf_profiler* saf_profiler_create(int32_t capacity_pairs);
void saf_profiler_destroy(saf_profiler* p);
void saf_profiler_reset(saf_profiler* p);
/* record only every stride-th frame of a saf_fuse_frames_profiled call (event packets between the
 * kernels cost a few microseconds each; 1 = every frame) */
void saf_profiler_set_stride(saf_profiler* p, int32_t stride);
/* total elapsed ms and number of launches recorded for one kernel class; <0 on error */
int saf_profiler_read(saf_profiler* p, int32_t kernel_class, double* total_ms, int64_t* launches);

/* saf_fuse_frames with event pairs recorded into `profiler` (may be NULL = no recording; pairs
 * beyond the pool's capacity are silently not recorded). */
int saf_fuse_frames_profiled(const saf_volume* vol, const saf_frame* frames, int32_t n_frames,
                             void* workspace, size_t workspace_bytes, uint64_t* stats,
                             saf_profiler* profiler, void* stream);

/* saf_fuse_frames_profiled into a recycled volume (see saf_clear_unwritten_rows), then saf_clear_unwritten_rows over all of
 * it, as ONE call: when it has completed (stream order) every voxel whose weight is 0 has a zero row, whatever the rows held before.  The reference builds a
 * new, zeroed module per scan (clip_seem_fusion.py:291-302); this is that scan's fusion with the 4*D*N-byte clear folded in: in
 * the windowed path the zeros are written beside the last window's row kernel (which leaves most of the HBM bandwidth unused)
 * and only where no frame of the call wrote; any other path zeroes the rows first.  profiler may be NULL.  n_frames == 0: the clear
 * alone. */
int saf_fuse_frames_recycled(const saf_volume* vol, const saf_frame* frames, int32_t n_frames, void* workspace,
                             size_t workspace_bytes, uint64_t* stats, saf_profiler* profiler, void* stream);

/* saf_fuse_frames slab by slab (new capability: the frame-sharded multi-GPU job with its merge pipelined behind the fusion,
 * SURVEY 8e): EVERY frame is fused into x-planes [slab_x0[k], slab_x0[k] + slab_nx[k]) of the volume for k = 0 .. n_slabs - 1
 * in turn -- a slab of x-planes is a contiguous range of the flat voxel index and every decision is that of the full volume's
 * voxels (clipfusion.py:617-622: the same axis table), so the slabs together equal saf_fuse_frames bit for bit; a finished
 * slab is never touched again.  slab_done_events (may be NULL, entries may be NULL): hipEvent_t handles, event k is recorded
 * on `stream` behind the last kernel that writes slab k -- the caller's reduce-scatter of that slab waits for it on its own
 * stream.  One call: the first window of slab k + 1 is classified beside the last row kernel of slab k.  Slabs must not
 * overlap; multiples of 16 x-planes keep the fast unit orders.  profiler may be NULL.  recycled != 0: the volume is a recycled
 * one (saf_fuse_frames_recycled) -- the rows of a slab that are still unwritten are zeroed behind the slab's last row kernel,
 * before its event; voxels outside every slab are not touched. */
int saf_fuse_frames_slabs(const saf_volume* vol, const saf_frame* frames, int32_t n_frames, const int32_t* slab_x0,
                          const int32_t* slab_nx, int32_t n_slabs, void* const* slab_done_events, int32_t recycled,
                          void* workspace, size_t workspace_bytes, uint64_t* stats, saf_profiler* profiler, void* stream);

/*
 * Depth un-projection of a lattice of pixels to world points: the per-frame body of
 * backproject_pcd (clipfusion.py:541-565) with get_pix_vecs (:497-507) folded in.
 *   u_idx[nu], v_idx[nv] : pixel columns / rows of the lattice (device i32)
 *   Kinv                 : [3,3] inverse intrinsics (device f32; the host inverts K)
 * Writes xyz[nv*nu,3] (world), valid[nv*nu] (u8: depth not NaN, >0, <max_depth) in lattice order
 * (v-major, as meshgrid(xy).view(-1) orders it).
 */
int saf_backproject_lattice(const float* depth, int32_t height, int32_t width, const float* pose,
                            const float* Kinv, const int32_t* u_idx, int32_t nu,
                            const int32_t* v_idx, int32_t nv, float max_depth, float* xyz,
                            uint8_t* valid, void* stream);

/* Epilogues of the text-query scan. */
enum saf_query_epilogue {
  SAF_Q_SCORES = 0,  /* out[n,l] = scale * <f_n, t_l>                                   */
  SAF_Q_SOFTMAX = 1, /* Clip.run_query, clipfusion.py:899-904: softmax_l(scale*<f_n,t_l>) */
  SAF_Q_SURGERY = 2  /* Clip.clip_feature_surgery (redundant_feats=None), clipfusion.py:911-932:
                        out[n,l] = S[n,l]*w[l] - mean_l(S[n,l]*w[l]), w from row 0 of feats */
};

/* Row normalisation applied to the features before the dot products. */
enum saf_query_normalize {
  SAF_NORM_NONE = 0,
  SAF_NORM_L2 = 1,       /* f / |f|, NaN -> 0 (clip_seem_fusion.py:507-511; query_mesh.py:24-25) */
  SAF_NORM_L2_CLAMP = 2  /* f / max(|f|, 0.1) (eval_scannet_segmentation.py:549-551, hypersim_eval.py:50-51) */
};

/*
 * Scan n_rows feature rows against n_text text embeddings.
 *   feats      [n_rows, feat_stride] feat_dtype (row-major; first D columns used)
 *   text       [n_text, text_stride] f32 (first D columns used: run_query truncates, :901)
 *   normalize  a saf_query_normalize: SAF_NORM_L2 divides each row by its L2 norm first and maps NaN -> 0
 *              (clip_seem_fusion.py:507-511; query_mesh.py:24-25 without the nan_to_num); SAF_NORM_L2_CLAMP
 *              divides by max(norm, 0.1) as the eval scripts do
 *   out        [n_rows, n_text] f32
 *   out_last   optional [n_rows] f32: only the last column (query_mesh.py:38); out may be NULL then
 *   workspace  device scratch of saf_query_workspace_bytes(n_text, epilogue) bytes (may be NULL if 0)
 * Numerics (ABI 3, round 6): for feat_dim % 16 == 0 and up to 64 labels (or more, 64 / 32 at a time, when `out` is given) the dot
 * products run on fp16 matrix instructions with fp32 accumulation -- fp32 operands cut into two fp16 pieces under power-of-two
 * scales (per label; per feature row, following the row's running maximum), 16-bit features as one piece: a score is within
 * 3 x 2^-22 of sum_k |f_k t_k| of the exact dot product for rows and labels of any magnitude the dtype holds (the reference's scores
 * are compared at 1e-4).  SAF_Q_SPLIT=0 in the environment (read per call): the exact-fp32 matrix instructions instead.
 *
 * Rows with an inf or a NaN in them (fp16 fusion can leave them: SAF_F16 above) -- a row is "bad" when it holds an inf or a NaN.
 * On every route of the dispatch (one wave per row, the exact-fp32 and the split matrix scans, blocks of labels with their
 * finishing pass), for `out` and for `out_last`:
 *   SAF_NORM_L2        a bad row is the all-zero row (clip_seem_fusion.py:507-511, nan_to_num of f / |f|): SAF_Q_SCORES gives 0.0
 *                      in every column, SAF_Q_SOFTMAX 1 / n_text, SAF_Q_SURGERY 0.0 (the zero row's value); a bad row 0 gives the
 *                      surgery weights of the zero row (every weight 1);
 *   SAF_NORM_NONE, SAF_NORM_L2_CLAMP   no nan_to_num in the reference: every output of a bad row is the IEEE result and not
 *                      finite.  Whether it is NaN or an infinity depends on the route (the split scans cut an inf into the pieces
 *                      hi = inf, lo = NaN and give NaN where exact arithmetic has an infinity); an infinity has the exact
 *                      result's sign;
 *   in every mode all other rows' outputs are bit for bit what they are without the bad rows, and out_last is the last column of
 *   the same call bit for bit.
 * Not covered by this rule: finite rows whose fp32 sum of squares overflows or underflows (the factor 1 / |f| is then 0 or
 * infinite where the exact norm is not), and text rows that are not finite.
 */
int saf_query_scan(const void* feats, int32_t feat_dtype, int64_t n_rows, int64_t feat_stride,
                   int32_t feat_dim, const float* text, int32_t n_text, int64_t text_stride,
                   int32_t epilogue, float scale, int32_t normalize, float* out, float* out_last,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Device scratch saf_query_scan needs (the surgery weights w[n_text]); 0 for other epilogues. */
size_t saf_query_workspace_bytes(int32_t n_text, int32_t epilogue);

/*
 * Top-k labels per row (ABI 4; eval_scannet_segmentation.py:546-561 -- `segment`, of whose argsort the eval reads columns [:, :5]
 * and [:, 0]): per row the k labels of largest scale * <f^, t_l>, best first, f^ the row under `normalize` (the eval: SAF_NORM_L2_CLAMP,
 * scale 100).  Of equal scores the smaller label comes first.
 *   feats / text / normalize as saf_query_scan; n_text >= 1
 *   k          1 <= k <= 8 and k <= n_text (SAF_E_INVALID otherwise)
 *   out_index  [n_rows, k] i32
 *   out_prob   [n_rows, k] f32 or NULL: the labels' softmax probabilities over ALL n_text labels (the reference's `relevance`)
 *   workspace  saf_query_topk_workspace_bytes(n_rows, n_text, k) bytes, 256-byte aligned (0 for n_text <= 32): the rows' running
 *              top-k and softmax maximum / denominator between blocks of 64 (32 at feat_dim > 512) labels
 * Numerics as saf_query_scan: the split scan for feat_dim % 16 == 0 (SAF_Q_SPLIT=0: exact fp32), exact fp32 matrix instructions for
 * feat_dim % 8 == 0; other widths (or rows not on 16-byte boundaries) one wave per row, fp32.
 *
 * Rows with an inf or a NaN in them ("bad" rows, as at saf_query_scan), on every route:
 *   SAF_NORM_L2        a bad row is the all-zero row: every score is 0, so out_index is 0 .. k - 1 in that order (equal scores: the
 *                      smaller label first) and out_prob is fp32(1) / fp32(n_text) each, within one fp32 ulp;
 *   SAF_NORM_NONE, SAF_NORM_L2_CLAMP   the scores are the IEEE results.  A NaN score is never chosen: a row whose scores are all
 *                      NaN reports out_index -1 and out_prob 0 in all k places.  Any other bad row reports labels in [-1, n_text),
 *                      none of them twice (-1 where fewer than k scores are not NaN); its out_prob need not be finite;
 *   in every mode all other rows' labels and probabilities are bit for bit what they are without the bad rows.
 * Not covered: finite rows whose fp32 sum of squares overflows or underflows, and text rows that are not finite.
 */
size_t saf_query_topk_workspace_bytes(int64_t n_rows, int32_t n_text, int32_t k);
int saf_query_topk(const void* feats, int32_t feat_dtype, int64_t n_rows, int64_t feat_stride, int32_t feat_dim, const float* text,
                   int32_t n_text, int64_t text_stride, float scale, int32_t normalize, int32_t k, int32_t* out_index,
                   float* out_prob, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Exact nearest neighbour (ABI 4; eval_scannet_segmentation.py:585-586, scipy.spatial.KDTree(pred).query(gt)): for every query
 * point the reference point of smallest squared distance, computed in fp64 from the fp32 coordinates ((qx-rx)^2 + (qy-ry)^2 +
 * (qz-rz)^2 in that order); of equal distances the smaller reference index.
 *   ref        [n_ref, 3] f32, n_ref >= 1;  query [n_query, 3] f32 (n_query = 0: nothing to do)
 *   out_index  [n_query] i32;  out_dist2 [n_query] f64 or NULL
 *   workspace  saf_nearest_workspace_bytes(n_ref, n_query) bytes, 256-byte aligned
 * Method: a uniform grid over the reference points' bounding box (at most n_ref cells, sized on the device: no host
 * synchronisation), the points counting-sorted into cells, each query searching rings of cells outward until no unsearched cell
 * can hold a point as near.  Coordinates must be finite (the Python layer checks); any input stays in bounds.
 */
size_t saf_nearest_workspace_bytes(int64_t n_ref, int64_t n_query);
int saf_nearest_points(const float* ref, int64_t n_ref, const float* query, int64_t n_query, int32_t* out_index, double* out_dist2,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * Segmentation scoring counts (ABI 4; eval_scannet_segmentation.py:589-601 and sklearn's confusion_matrix(labels=range(L))):
 *   gt         [n] i32 ground-truth class per vertex; a vertex with gt outside [0, n_classes) (-1: unlabelled) is skipped
 *   pred       [n, pred_stride] i32 predicted labels, best first; topk <= pred_stride
 *   cmat       [n_classes, n_classes] i64: cmat[g, p0] += 1 (p0 = pred[i, 0]; a p0 outside [0, n_classes) is left out of cmat only)
 *   ncorrect_top1 / ncorrect_topk / ntotal  [n_classes] i64: p0 == g / g among the first topk / every counted vertex
 *   accumulate 0: the outputs are zeroed first; otherwise the counts are added to them (a confusion matrix over many scenes)
 * Exact integer counts, independent of scheduling.
 */
int saf_segmentation_counts(const int32_t* gt, const int32_t* pred, int64_t n, int32_t pred_stride, int32_t topk, int32_t n_classes,
                            int64_t* cmat, int64_t* ncorrect_top1, int64_t* ncorrect_topk, int64_t* ntotal, int32_t accumulate,
                            void* stream);

/*
 * Wide scan (BASELINE config 5: hundreds to thousands of text queries over a 16-bit feature
 * volume): scores out[n,q] = scale * <f_n, t_q> (rows optionally L2-normalised first) on the 16-bit
 * matrix cores with fp32 accumulation.  The text embeddings are rounded to the feature dtype.
 *   feats      [n_rows, feat_stride] SAF_F16 or SAF_BF16, feat_dim in {128, 256, 512}
 *   out        [n_rows, out_stride] of out_dtype (SAF_F32, SAF_F16 or SAF_BF16), out_stride >= n_text
 *   workspace  saf_query_wide_workspace_bytes(n_text, feat_dim) bytes of device scratch
 * Strides, the columns of `out` that are written and rows with inf / NaN in them: see saf_query_scan_wide_ex below.
 */
size_t saf_query_wide_workspace_bytes(int32_t n_text, int32_t feat_dim);
int saf_query_scan_wide(const void* feats, int32_t feat_dtype, int64_t n_rows, int64_t feat_stride,
                        int32_t feat_dim, const float* text, int32_t n_text, int64_t text_stride,
                        float scale, int32_t normalize, void* out, int32_t out_dtype, int64_t out_stride,
                        void* workspace, size_t workspace_bytes, void* stream);

/*
 * Wide scan with fused epilogues (64 feature rows per wave at one wave per SIMD; feat_dim 256 or 512).  BASELINE
 * config 5's N x Q score matrix (33 GB at 256^3 x 1000 fp16) is twice the volume it is computed from; the
 * reductions the reference's callers apply to it are fused here:
 *   SAF_QW_SCORES         out[n, q] = scale * <f_n, t_q>                         (as saf_query_scan_wide)
 *   SAF_QW_VS_BACKGROUND  the first n_background text rows are shared background prompts, the others targets:
 *                         out[n, t] = softmax(scale * [<f_n, bg_0..>, <f_n, target_t>])[-1] -- query_mesh.py:36-39 and
 *                         hypersim_eval.py:76-81 for every target at once; flags & 1 adds query_mesh.py:39's
 *                         ((r - 0.5) * 2).clamp(0, 1).  out is [n_rows, n_text - n_background].
 *   SAF_QW_ROW_ARGMAX     per row the best query and its score: out_index[n] i32, out_value[n] f32
 *                         (eval_scannet_segmentation.py:553-560: the first label of the argsort); nothing N x Q is written.
 *                         The dot products are compared before the row's scale / norm is applied (one factor per row;
 *                         a negative scale is folded into the text): of equal products the first query wins.
 *   SAF_QW_QUERY_MAX      per query the best row and its score: out_value[q] f32, out_row[q] i64 = row_offset + local
 *                         row (equal scores: the smaller row), -1 / -inf when n_rows = 0; row_offset lets ranks that
 *                         scan voxel shards report global voxel indices.
 * Unused outputs may be NULL.  workspace: saf_query_wide_ex_workspace_bytes(...) bytes, 256-byte aligned.
 *
 * Layout (both entry points): feats on 16 bytes and feat_stride a multiple of 8 elements, >= feat_dim; text_stride >= feat_dim;
 * `out` at any element-aligned base and any out_stride >= its columns (n_text; VS_BACKGROUND: n_text - n_background).  On a
 * 16-byte base saf_query_scan_wide_ex stores 16 bytes at a time when out_stride is a multiple of 8 elements, and
 * saf_query_scan_wide four scores at a time (16 bytes of fp32, 8 bytes of 16-bit output) when it is a multiple of 4; anything else
 * is stored element by element: the values are the same.  Only columns [0, columns) of each of the n_rows rows are written;
 * whatever lies between the rows stays as it was.
 *
 * Rows with an inf or a NaN in them (fp16 fusion can leave them: SAF_F16 above) -- a row is "bad" when its fp32 sum of squares is
 * not finite:
 *   SAF_NORM_L2        a bad row is the all-zero row (clip_seem_fusion.py:507-511, nan_to_num of f / |f|): score 0 in every
 *                      column, ROW_ARGMAX gives (0, 0.0), and it takes part in QUERY_MAX with score 0;
 *   SAF_NORM_NONE, SAF_NORM_L2_CLAMP   no nan_to_num in the reference: a bad row's scores are the IEEE result, NaN or +-inf;
 *   in every mode all other rows' outputs are bit for bit what they are without the bad rows.
 * A NaN score never wins a reduction, wherever its row lies: QUERY_MAX is the maximum over the scores that are not NaN (an infinite
 * score is a score and wins; equal scores: the smaller row); ROW_ARGMAX of a row is its first maximum over the scores that are not
 * NaN (a row of NaN scores only: an index in [0, n_text), the value not finite).  A query all of whose scores are NaN or -inf
 * reports -inf and no particular row.
 */
enum saf_wide_epilogue { SAF_QW_SCORES = 0, SAF_QW_VS_BACKGROUND = 1, SAF_QW_ROW_ARGMAX = 2, SAF_QW_QUERY_MAX = 3 };
size_t saf_query_wide_ex_workspace_bytes(int32_t n_text, int32_t feat_dim, int32_t epilogue, int32_t n_background);
int saf_query_scan_wide_ex(const void* feats, int32_t feat_dtype, int64_t n_rows, int64_t feat_stride,
                           int32_t feat_dim, const float* text, int32_t n_text, int64_t text_stride, float scale,
                           int32_t normalize, int32_t epilogue, int32_t n_background, int32_t flags, void* out,
                           int32_t out_dtype, int64_t out_stride, int32_t* out_index, float* out_value,
                           int64_t* out_row, int64_t row_offset, void* workspace, size_t workspace_bytes, void* stream);

/*
 * After the cross-rank SUM of SAF_SUM-mode volumes: clip_feat <- F/w,
 * rgb <- C/w, tsdf <- T/wt over voxels [first, first+count); rows with zero weight stay zero.
 * More exactly: a row with w <= 0 (wt <= 0 for the tsdf) is not touched -- it keeps its bytes, whatever they are -- and every
 * scaled value is one IEEE fp32 division by (float)w.  Voxels outside the range are not touched.  SAF_F32 volumes only.
 */
int saf_merge_finalize(const saf_volume* vol, int64_t first_voxel, int64_t n_voxels, void* stream);

/* Inverse of the above for a volume that was fused in SAF_RUNNING_MEAN mode: mean -> sum
 * (x*w), so that it can enter the reduction.  The product is taken in EVERY row of the range, one fp32 multiplication by
 * (float)w: a row with w == 0 becomes x * 0 -- zero where it held finite data (by the volume's contract it held zeros), NaN where
 * it held NaN or inf.  The round trip mean -> sum -> mean moves a value by at most one unit in the last place where w > 0. */
int saf_mean_to_sum(const saf_volume* vol, int64_t first_voxel, int64_t n_voxels, void* stream);

/*
 * The PACKED route of the frame-sharded merge (new capability, nothing to mirror in the reference): after
 * the all-reduce of `weight` every rank knows which rows ANY rank touched; of a piece whose touched share is small only those
 * rows travel (all_to_all with uneven splits, issued by the host: spatially_aware_ai_amd/distributed.py).  Rows are indexed
 * relative to the first row of the slab / volume being merged; `weight` and `pos` cover the same rows.
 *   saf_merge_scan_touched  pos[i] = number of touched rows (weight > 0) among [0, i), i = 0 .. n_rows (n_rows + 1 words), and
 *                           offs_host[j] = pos[bounds[j]] (bounds: device memory; offs_host: host memory, pinned for an
 *                           asynchronous copy) -- the split sizes of the collective; the caller synchronises the stream once
 *                           before reading them.  workspace: saf_merge_scan_workspace_bytes(n_rows, n_bounds).
 *   saf_merge_pack_rows     the touched rows of [first, first + n_rows) of `src` (rows of row_bytes bytes, a multiple of 4) ->
 *                           packed[pos[r] - pos[first]]: the send buffer, touched rows in ascending order.
 *   saf_merge_add_packed    dst[r] = recv[0][p] + recv[1][p] + ... + recv[world - 1][p] (rank order: deterministic) for the
 *                           touched rows r of [first, first + n_rows), p = pos[r] - pos[first]; recv = [world][mine] rows as
 *                           all_to_all_single leaves them; is_float: f32 rows (else i32).
 */
size_t saf_merge_scan_workspace_bytes(int64_t n_rows, int32_t n_bounds);
int saf_merge_scan_touched(const int32_t* weight, int64_t n_rows, int32_t* pos, const int64_t* bounds, int32_t n_bounds,
                           int32_t* offs_host, void* workspace, size_t workspace_bytes, void* stream);
int saf_merge_pack_rows(const void* src, int64_t row_bytes, const int32_t* weight, const int32_t* pos, int64_t first,
                        int64_t n_rows, void* packed, void* stream);
int saf_merge_add_packed(void* dst, int64_t row_bytes, int32_t is_float, const int32_t* weight, const int32_t* pos, int64_t first,
                         int64_t n_rows, const void* recv, int64_t mine, int32_t world, void* stream);

/*
 * A fused volume carried into another box of the SAME lattice (additive under ABI 7; new capability, nothing to mirror in the
 * reference: its manager re-fuses every frame of a scan into a new grid when the scan grows, get_path(config, curr_ver, ...)).
 * `src` and `dst` are two boxes of one lattice -- same origin, same voxel size, corners that differ by whole voxels -- so the pass
 * is a copy and nothing is recomputed (blending two volumes of one lattice: saf_volume_absorb below;
 * coarsening by a whole factor on block boundaries of the lattice: saf_volume_coarsen below; resampling onto any other lattice
 * -- rotated, a fractional factor, finer -- under a rigid transform: saf_volume_resample below).
 *   mapping   destination voxel (x, y, z) corresponds to source voxel (x + off_x, y + off_y, z + off_z); the caller passes
 *             off = dst's index offset - src's.  The OVERLAP is the set of destination voxels whose source voxel lies inside
 *             `src`.  A destination voxel outside the overlap is not touched: every buffer keeps its bytes there.
 *   copied    per overlap voxel: tsdf, tsdf_weight, weight, the three rgb floats, and aux_src -> aux_dst ([N_src] / [N_dst] i32,
 *             an optional pair: whatever the caller keeps per voxel, e.g. an object index).  If and only if the source `weight`
 *             is > 0, also the feature row and, with n_classes > 0, the label histogram row.  Bytes are copied, whatever the
 *             dtype (SAF_F32, SAF_BF16, SAF_F16; any feat_dim).
 *   not read  the feature / label row of a source voxel with weight == 0: after a deferred clear (saf_clear_unwritten_rows still
 *             owed) it holds stale data, which the windowed fuse path never reads either.  The destination row of such a voxel
 *             is NOT WRITTEN: the caller supplies a destination whose weight-0 rows are zero, or owes it the same clear.
 *             The axis tables, accum_mode and trunc of the two descriptors are not inspected: a copy is a copy.
 *   counts    device u64[2], ADDED to (may be NULL): [0] += overlap voxels with weight > 0 (rows carried), [1] += overlap voxels
 *             with tsdf_weight > 0.  Integer atomics: exact whatever the scheduling.
 * SAF_E_INVALID (on the host, nothing is launched) for a NULL src / dst or a NULL tsdf, tsdf_weight, weight, rgb or clip_feat (or
 * labels_one_hot with n_classes > 0), non-positive sizes or feat_dim, a grid of 2^31 voxels or more, feat_dim, feat_dtype or
 * n_classes that differ between the two, only one of aux_src / aux_dst, and any destination buffer whose byte range intersects
 * the source buffer of the same name (the pass works out of place only).  An empty overlap is SAF_OK with nothing launched.
 * One launch; a wave takes 64 consecutive voxels of the flattened overlap box and copies the touched rows one after the other,
 * 16 bytes per lane where the row pitch and both bases allow it, else 4 (the 572-byte label rows) or 2.  Per call
 * 28 N_overlap + M (row_bytes + label_row_bytes) bytes are read and as many written, M = counts[0].
 */
int saf_volume_carry(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z,
                     const int32_t* aux_src, int32_t* aux_dst, uint64_t* counts, void* stream);

/*
 * A second fused volume of the SAME lattice absorbed into this one: blended by weights (additive under ABI 7; new capability,
 * nothing to mirror in the reference, which fuses every frame of the second scan again).  Mapping and
 * overlap are saf_volume_carry's: destination voxel (x, y, z) corresponds to source voxel (x + off_x, y + off_y, z + off_z), the
 * caller passes off = dst's index offset - src's.  `dst` is updated IN PLACE over the overlap; outside it no byte of `dst` changes;
 * `src` is only read.  Both volumes are running means (SAF_RUNNING_MEAN) of the same truncation distance: the pass does not
 * inspect trunc or the axis tables.
 *   per voxel  the feature side (ws, wd = the source's and the destination's `weight`; it owns weight, the three rgb floats, the
 *             feature row and, with n_classes > 0, the label histogram row) and the TSDF side (`tsdf_weight`; it owns tsdf_weight
 *             and tsdf) are treated independently, by the same three cases:
 *   ws == 0   nothing of that side is written: the destination keeps its bytes, whatever they are.  The source's row is not read
 *             (after a deferred clear it holds stale data).
 *   wd == 0   (ws > 0) a copy, as in carry: the destination takes the source's bytes.  The destination's old row is NOT READ:
 *             after a deferred clear it is stale, and a weight-0 row that is never written stays owed that clear.
 *   blend     (ws > 0, wd > 0) w' = wd + ws (int32; not checked for overflow: these are frame counts), r = 1.0f / (float)w' by
 *             IEEE division, cs = (float)ws * r, cd = (float)wd * r, and every rgb and feature channel (and tsdf) becomes
 *             x' = xs * cs + xd * cd: two separately rounded products, one rounded sum, no FMA.  16-bit rows (SAF_BF16, SAF_F16)
 *             are widened exactly, computed in fp32 and narrowed with one round-to-nearest-even.  The label histogram is an int32
 *             add.  weight = w'.  NaN and inf travel as IEEE arithmetic carries them.  With ws == 1 this is the running-mean step
 *             of saf_fuse_frames for weight, rgb, feature rows and labels; the forward sweep's TSDF uses the hardware reciprocal
 *             and so differs from this one by rounding (the TSDF is compared at 1e-4 throughout).
 *   counts    device u64[4], ADDED to (may be NULL): [0] rows blended, [1] rows copied, [2] tsdf voxels blended, [3] tsdf voxels
 *             copied.  Integer atomics, one per wave and counter: exact whatever the scheduling.
 * SAF_E_INVALID (on the host, nothing is launched) for everything saf_volume_carry refuses -- a NULL src / dst or volume buffer,
 * non-positive sizes or feat_dim, a grid of 2^31 voxels or more, feat_dim, feat_dtype or n_classes that differ, any destination
 * buffer whose byte range intersects the source buffer of the same name -- and for a feature or label buffer that is not aligned
 * to its element type.  SAF_E_UNSUPPORTED if either accum_mode is SAF_SUM.  An empty overlap is SAF_OK with nothing launched.
 * One launch, carry's shape: a wave takes 64 consecutive voxels of the flattened overlap box, two ballots name the rows to copy and
 * the rows to blend, and the wave takes them one after the other, 16 bytes per lane where the row pitch and both bases allow it,
 * else 4 or 2; a blended row's loads (both rows) are issued before its arithmetic.  No LDS, no scratch, no floating-point atomics.
 * Per call 28 N_overlap bytes are read from each volume and at most 28 N_overlap written; per copied row one row (feature + label
 * bytes) is read and one written, per blended row two are read and one written.
 */
int saf_volume_absorb(const saf_volume* src, const saf_volume* dst, int32_t off_x, int32_t off_y, int32_t off_z,
                      uint64_t* counts, void* stream);

/*
 * A fused volume coarsened by a whole factor f = 2, 3 or 4 on BLOCK BOUNDARIES OF ITS LATTICE (additive under ABI 7; new
 * capability, nothing to mirror in the reference, which pushes every frame through the backbones again into a coarser grid;
 * DESIGN.md section 4.21).  A coarse voxel is the weighted mean of the f^3 fine voxels it covers: saf_volume_absorb's blend with
 * up to f^3 sources instead of two.  `src` is only read; `dst` is another set of buffers (the pass works out of place only).
 *   mapping   `src` holds its nx x ny x nz voxels from global index off = (off_x, off_y, off_z) of the lattice (origin, vs).  Global
 *             coarse voxel I (per axis) covers the fine global indices f I .. f I + f - 1 -- a FLOOR division, so negative offsets
 *             work and blocks are aligned to the lattice, not to the box.  The coarse lattice has voxel_size' = f vs and origin' =
 *             origin + 0.5 (f - 1) vs, the centre of the block of global coarse index 0 (the caller computes it in float64 and
 *             stores it as origin was stored); index_offset' = floor(off / f) and nvox' = ceil((off + n) / f) - floor(off / f) per
 *             axis: `dst` must have exactly these sizes.  trunc does not change (TSDF values are in units of trunc).  Children of
 *             an edge block that lie outside the fine box count as empty.  origin' depends on origin, vs and f only: two boxes of
 *             one fine lattice coarsen to two boxes of one coarse lattice.  The pass does not inspect trunc or the axis tables.
 *   per voxel  two independent sides, as in absorb: the feature side (driven by `weight`; it owns weight, the three rgb floats, the
 *             feature row and, with n_classes > 0, the label histogram row) and the TSDF side (driven by `tsdf_weight`; it owns
 *             tsdf_weight and tsdf).  Children are visited in ascending fine flat index (x slowest, z fastest); K = the number
 *             of children with w_c > 0, W = their sum (int32; not checked for overflow: these are frame counts).
 *   K == 0    the small fields of that side are written 0; the feature and label rows are NOT WRITTEN: the caller supplies a
 *             destination whose weight-0 rows are zero, or owes it the deferred clear (saf_clear_unwritten_rows).
 *   K == 1    a copy of that child's bytes (values, row, labels): w fl(1 / w) is not 1 for every w, so the copy is its own case,
 *             as in absorb.
 *   K >= 2    r = 1.0f / (float)W by IEEE division, c_k = (float)w_k * r, acc = x_1 * c_1 for the first contributing child, then
 *             acc = acc + x_k * c_k in order: every product and every sum rounded on its own, no FMA.  For each rgb channel and each
 *             feature channel, and for tsdf with the tsdf_weights.  16-bit rows (SAF_BF16, SAF_F16) are widened exactly,
 *             accumulated in fp32 and narrowed ONCE, round to nearest even.  The label histogram is the int32 sum over the
 *             contributing children only.  NaN and inf in contributing rows travel as IEEE arithmetic carries them.
 *   counts    stored: weight' = max_c w_c and tsdf_weight' = max_c w_c, NOT the sum.  The blend uses every sample; the stored count
 *             stands for "frames that saw this block", which lies between the max and the sum (one frame usually sees several
 *             children of a block), and the max keeps a later frame's sample worth one frame in the running mean that goes on.
 *   not read  the values and rows of a child with w_c == 0 (stale after a deferred clear, possibly NaN), and everything outside `src`.
 *   bias      a block whose observed children all lie on one side of its centre gets a TSDF that is off by up to half a coarse
 *             voxel (known, documented, not corrected); the mean of a linear field over all f^3 children is its value at the centre.
 *   counts[]  device u64[4], ADDED to (may be NULL): [0] rows blended (K >= 2), [1] rows copied (K == 1), [2] tsdf voxels blended,
 *             [3] tsdf voxels copied.  Integer atomics, one per wave and counter: exact whatever the scheduling.
 * SAF_E_INVALID (on the host, nothing is launched) for everything saf_volume_carry refuses -- a NULL src / dst or volume buffer,
 * non-positive sizes or feat_dim, a grid of 2^31 voxels or more, feat_dim, feat_dtype or n_classes that differ, any destination
 * buffer whose byte range intersects the source buffer of the same name --, for a feature or label buffer that is not aligned to
 * its element type, for a factor outside 2 .. 4 and for a `dst` whose nx, ny, nz are not the nvox' of `src` under the off passed.
 * SAF_E_UNSUPPORTED if either accum_mode is SAF_SUM.
 * One launch, carry's and absorb's shape: a wave takes 64 consecutive voxels of the flattened coarse box (z fastest: the children
 * along z are adjacent); each lane computes its block's small fields; a ballot names the blocks with a row to write and the wave
 * takes them one after the other: lane j looks up child j (f^3 <= 64), a ballot over their counts names the contributing
 * children, and their indices and coefficients are read from those lanes; 16 bytes per lane where the row pitch and both bases
 * allow it, else 4 or 2; the loads of up to 8 children are issued before their arithmetic.  No LDS, no scratch, no floating-point
 * atomics.  Per call 8 N_src bytes of counts are read and 12 / 4 more per fine voxel with weight / tsdf_weight > 0, 28 N_dst bytes
 * are written; per contributing child one row (feature + label bytes) is read, per coarse voxel with K >= 1 one is written.
 */
int saf_volume_coarsen(const saf_volume* src, const saf_volume* dst, int32_t factor, int32_t off_x, int32_t off_y, int32_t off_z,
                       uint64_t* counts, void* stream);

/*
 * A fused volume resampled onto ANY OTHER lattice under a rigid transform -- rotated, shifted by a fraction of a voxel, finer,
 * coarser by any factor (additive under ABI 7; new capability, nothing to mirror in the reference, which pushes every frame
 * through the backbones again into the other grid).  A PULL resample: every destination voxel looks up the
 * eight source voxels around its own centre and blends the observed ones by their trilinear weights, renormalised.  `src` is only
 * read; `dst` is another set of buffers (the pass works out of place only).
 *   mapping   m12 (HOST memory, row-major 3 x 4, read during the call) takes a destination voxel's local index (x, y, z) to a
 *             continuous local source index p.  The caller builds it in float64 and rounds it once to f32: from the centre
 *             world_new = (i + off_dst) vs_dst + origin_dst, world_old = inv(T) world_new for the rigid 4 x 4 T = new_from_old, and
 *             p = (world_old - origin_src) / vs_src - off_src.  On the device, per axis a,
 *             p_a = ((m_a0 (float)x + m_a1 (float)y) + m_a2 (float)z) + m_a3: four roundings, no FMA.  If p_a < -1 or
 *             p_a >= (float)n_a on any axis -- compared in float before any conversion -- the voxel has no corner.  Otherwise
 *             i_a = floorf(p_a) and f_a = p_a - (float)i_a (f_a may round to 1.0 for a tiny negative p_a: harmless).  The pass
 *             does not inspect trunc or the axis tables; trunc does not change (TSDF values are in units of trunc), so a T that
 *             scales is the caller's to refuse.
 *   corners   corner k = 4 dx + 2 dy + dz (ascending source flat index) is source voxel (i_x + dx, i_y + dy, i_z + dz); its
 *             trilinear weight is t_k = (a_x * a_y) * a_z with a = f_a where the corner's bit is 1 and 1.0f - f_a where it is 0.
 *   per voxel  two independent sides, as in absorb and coarsen: the feature side (driven by `weight`; it owns weight, the three rgb
 *             floats, the feature row and, with n_classes > 0, the label histogram row) and the TSDF side (driven by `tsdf_weight`;
 *             it owns tsdf_weight and tsdf).  On each side a corner CONTRIBUTES if it lies inside the source box, its count is
 *             > 0 and t_k > 0.  K = the number of contributing corners, S = the f32 sum of their t_k in ascending k, starting
 *             from the first contributing one.
 *   gate      the side is observed at this voxel iff K >= 1 and S >= min_cover (0 < min_cover <= 1; 0.5 is the module's default):
 *             without the gate one faint corner (t = 0.01) would carry its value a whole voxel outward and every surface would
 *             grow a fringe.  Not observed: the small fields of that side are written 0; the feature and label rows are NOT
 *             WRITTEN: the caller supplies a destination whose weight-0 rows are zero, or owes it the deferred clear
 *             (saf_clear_unwritten_rows).
 *   K == 1    (observed) a copy of that corner's bytes: values, row, labels.
 *   K >= 2    (observed) r = 1.0f / S by IEEE division, c_k = t_k * r, acc = x_1 * c_1 for the first contributing corner, then
 *             acc = acc + x_k * c_k in order: every product and every sum rounded on its own, no FMA.  For each rgb channel and
 *             each feature channel, and for tsdf on its own side.  16-bit rows (SAF_BF16, SAF_F16) are widened exactly,
 *             accumulated in fp32 and narrowed ONCE, round to nearest even.  The counts do NOT enter the coefficients: a count is
 *             confidence, not position, and weighting by it would pull an interpolated TSDF towards the better-seen corner.
 *   counts    stored: weight' = the maximum of the contributing corners' counts, and likewise tsdf_weight' (coarsen's rule and
 *             coarsen's reason: a later frame's sample stays worth one frame).
 *   labels    the label histogram row is COPIED from the contributing corner with the largest t_k, the lowest k on a tie -- not
 *             summed, which would multiply a voxel's votes by up to eight.
 *   not read  the values and rows of a corner that does not contribute (stale after a deferred clear, possibly NaN), and
 *             everything outside `src`.
 *   it follows  (a) with T the identity, equal lattices and a whole-voxel offset every observed voxel has one corner with t = 1,
 *             and the result is saf_volume_carry's into a zeroed destination, byte for byte; (b) a field that is linear in space
 *             is reproduced at the destination centres within rounding wherever all eight corners are observed: a plane's TSDF
 *             stays that plane's TSDF under any rotation and any voxel size (measured: at most 0.125 of the bound derived from
 *             the operation count in tests/resample_reference.py); (c) holes are not smeared: unobserved corners drop
 *             out and the rest are renormalised.  Trilinear interpolation low-passes the features by up to one source voxel
 *             (known, documented, not corrected).
 *   counts[]  device u64[4], ADDED to (may be NULL): [0] rows blended (observed, K >= 2), [1] rows copied (observed, K == 1),
 *             [2] tsdf voxels blended, [3] tsdf voxels copied.  Integer atomics, one per wave and counter.
 * SAF_E_INVALID (on the host, nothing is launched) for everything saf_volume_carry refuses -- a NULL src / dst or volume buffer,
 * non-positive sizes or feat_dim, a grid of 2^31 voxels or more, feat_dim, feat_dtype or n_classes that differ, any destination
 * buffer whose byte range intersects the source buffer of the same name --, for a feature or label buffer that is not aligned to
 * its element type, for a NULL m12 or one with an entry that is not finite, and for a min_cover outside (0, 1].
 * SAF_E_UNSUPPORTED if either accum_mode is SAF_SUM.
 * One launch, coarsen's shape: a wave takes 64 consecutive voxels of the flattened destination (z fastest); each lane computes its
 * voxel's p, corners, t_k and both sides' small fields; a ballot names the voxels with a row to write and the wave takes them one
 * after the other: the footprint, the contributing corners and r are read from the owning lane, the loads of all contributing
 * rows are issued before their arithmetic, 16 bytes per lane where the row pitch and both bases allow it, else 4 or 2.  No LDS, no
 * scratch, no floating-point atomics.  Per call up to 64 N_dst bytes of counts are read (8 per corner) and 12 / 4 more per
 * contributing corner, 28 N_dst bytes are written; per contributing corner of an observed voxel one feature row is read, per
 * observed voxel one label row is read and one row (feature + label bytes) is written.  Measured (DESIGN.md section 4.22;
 * 256^3 x 512 f32 into 256^3, 79 % touched): as a copy 11.1 ms, 1.12 x saf_volume_carry's time; rotated by 20 degrees 30.2 ms with
 * 7.1 rows read per row written, 3.07 x carry; the same arithmetic as torch gathers: 792 ms.
 */
int saf_volume_resample(const saf_volume* src, const saf_volume* dst, const float* m12, float min_cover, uint64_t* counts,
                        void* stream);

/*
 * Free-space carving: fused voxels that later frames SEE THROUGH are taken out of the volume again (additive under ABI 7; new
 * capability: the reference's integrate moves such a voxel's TSDF towards +1, clipfusion.py:678-679, and leaves its weight,
 * colour, features and label histogram alone, so an object that was carried out of the room stays in the volume for ever;
 * DESIGN.md section 4.23).  Two passes: saf_free_space_observe gathers the evidence, saf_volume_carve acts on it.
 *
 * saf_free_space_observe: for every voxel with weight > 0 and every frame of the call, the reference's classification of the voxel
 * centre (clipfusion.py:647-679) -- the projection, the nearest depth tap with zeros outside the image, sdf = (depth - z) / trunc,
 * in_view = |grid| <= 1 on both axes and z > 0, valid = in_view and |sdf| <= 1, tsdf_valid = in_view and sdf > -1: the operations
 * of the fuse path, whose decisions are pinned to the oracle's bit for bit -- and then
 *   seen[n] += the number of frames with tsdf_valid && !valid   (sdf > 1: the frame measured a surface BEHIND the voxel)
 *   hit[n]  += the number of frames with valid                  (the frame supports a surface at the voxel)
 * The counts are ADDED: a scan's frames may come over several calls, in any split and any order, with identical results.  The
 * entries of voxels with weight == 0 are neither read nor written.  The pass reads `weight`, `trunc` and the axis tables and
 * nothing else of the volume -- no feature row: a volume whose deferred clear is still owed is fine.  Depth values are taken as the
 * fuse path takes them: NaN gives neither count, +inf gives `seen`, and 0 or a negative value is a surface at or behind the camera
 * -- neither count for a voxel deeper than trunc, a hit for one nearer than that, exactly as the frame would be fused.
 *   depth [B,H,W], poses [B,4,4] (camera to world), K [B,3,3]: device f32, contiguous; seen, hit: device int32[nx ny nz].
 * One launch: a wave owns 64 consecutive voxels of the flattened grid (z fastest) and is their only writer (no atomics); a wave
 * with no touched voxel leaves at once; the frame loop is wave-uniform, a frame's pose and K are read through uniform addresses;
 * the counts stay in registers over the frames, then one load / add / store per touched voxel.  4 N bytes of weights are read,
 * per touched voxel and frame in view one depth tap, per touched voxel 16 bytes of evidence are read and written.
 *
 * saf_volume_carve: a voxel is carved iff weight > 0 && seen >= min_views && hit <= max_support.  A carved voxel becomes what a
 * fresh volume holds: weight, tsdf_weight, tsdf, the three rgb floats, the whole feature row and (n_classes > 0) the whole label
 * histogram row are set to zero bytes, so that fusing further frames gives, on a carved voxel, exactly what a fresh volume would
 * hold.  Every other byte of the volume is untouched; the evidence is only read, and of untouched voxels not even that.
 *   carved    device u8[N] (may be NULL): written 1 or 0 for EVERY voxel.
 *   counts[]  device u64[4], ADDED to (may be NULL): [0] voxels with weight > 0, [1] voxels carved, [2] voxels kept because
 *             hit > max_support although seen >= min_views, [3] voxels kept with 0 < seen < min_views.  Integer atomics, one per
 *             wave and counter.
 * One launch, saf_volume_carry's shape: each lane decides and zeroes its voxel's small fields, a ballot names the carved voxels
 * and the wave zeroes their rows one after the other, 16 bytes per lane where the row pitch and the base allow it, else 4 or 2.
 * No LDS, no scratch, no floating-point atomics.
 *
 * Both return SAF_E_INVALID on the host, with nothing launched, for a NULL volume, a NULL buffer they use (observe: weight, the
 * axis tables, depth, poses, K, seen, hit; carve: the six volume buffers, seen, hit), non-positive sizes (voxels per axis, batch,
 * height, width, feat_dim; a trunc that is not positive and finite), a grid of 2^31 voxels or more, an image of more than 2^31 - 1
 * pixels, min_views < 1, max_support < 0, an unknown feat_dtype, and a buffer that is not aligned to its element type; and
 * SAF_E_UNSUPPORTED for a SAF_SUM volume.
 * Left out: a margin beyond trunc (it would need its own float statement of sdf; the caller erodes the depth and asks for more
 * views instead), any policy that decides WHEN to carve, and taking carved frames out later (saf_unfuse_frames skips and counts a
 * voxel whose count is 0, as it always did).
 * Measured (256^3 x 512 f32; the coherent scene, 17 % touched / a 79 % touched volume): 128 frames of
 * 640 x 480 observed in 3.41 / 19.16 ms, against 376 ms for the reference's per-frame projection and masks in torch; the carve of
 * 0.59 M / 2.01 M voxels in 0.59 / 0.92 ms, 0.19 x / 0.09 x saf_volume_carry's time over the same volume, 11.6 ms as masked fills
 * in torch.
 */
int saf_free_space_observe(const saf_volume* vol, const float* depth, int32_t batch, int32_t height, int32_t width,
                           const float* poses, const float* K, int32_t* seen, int32_t* hit, void* stream);
int saf_volume_carve(const saf_volume* vol, const int32_t* seen, const int32_t* hit, int32_t min_views, int32_t max_support,
                     uint8_t* carved, uint64_t* counts, void* stream);

/*
 * Vertex sampling half of extract_mesh (clipfusion.py:741-760; clip_seem_fusion.py:843-878): for
 * marching-cubes vertices given in voxel-index coordinates, grid = (v + 0.5) * (1/nvox) * 2 - 1 and
 * 3-D grid_sample(align_corners=False, zeros padding) of the volume:
 *   out_feat [V,D] f32   trilinear sample of clip_feat (volume dtype f32, bf16 or fp16: 16-bit rows are widened exactly, one fp32 arithmetic)
 *   out_rgb  [V,3] f32   trilinear sample of rgb, clamped to [0,1]
 *   out_obj  [V]   f32   nearest sample of obj_idx [N] i32            (optional pair, may be NULL)
 *   out_seg  [V,3] f32   nearest sample of seg_color [N,3] f32, clamped (optional pair, may be NULL)
 */
int saf_sample_vertices(const saf_volume* vol, const float* verts_index, int64_t n_verts, float* out_feat,
                        float* out_rgb, const int32_t* obj_idx, float* out_obj, const float* seg_color,
                        float* out_seg, void* stream);

/*
 * The tiled CLIP front-end in one pass (Clip.img_inference_tiled before the ViT,
 * clipfusion.py:808-823): normalize_img, Unfold into overlapping patch x patch tiles at `stride`, bilinear resize of
 * every tile to out_size x out_size (align_corners = False).
 *   rgb    [batch, 3, H, W] f32 in 0..1 addressed through element strides (channel-last frames as the loaders yield
 *          them: stride_c = 1, stride_x = 3, stride_y = 3 W)
 *   mean3 / std3  HOST pointers to the three channel means / standard deviations (clipfusion.py:774-779)
 *   out    [batch * npy * npx, 3, out_size, out_size] of out_dtype, tile index (b * npy + py) * npx + px as
 *          get_patches orders them (clipfusion.py:800-804)
 */
int saf_clip_tiles(const float* rgb, int32_t batch, int32_t height, int32_t width, int64_t stride_b, int64_t stride_c,
                   int64_t stride_y, int64_t stride_x, int32_t patch, int32_t stride, int32_t out_size,
                   const float* mean3, const float* std3, void* out, int32_t out_dtype, void* stream);

/*
 * Ray cast of the fused volume from a camera pose (ABI 5; new capability, nothing to mirror in the reference: its AR client --
 * app_unity.py, magicleap2_camera_match.py -- asks what a headset camera sees of the volume).  One ray per pixel (u, v),
 * u = 0 .. width - 1, v = 0 .. height - 1; fp32 throughout, one IEEE operation at a time in the order written here
 * (tests/raycast_reference.py restates it in NumPy):
 *   grid     voxel centre i of an axis lies at axis[i]; origin = (axis_x[0], axis_y[0], axis_z[0]),
 *            voxel_size = (axis_x[nx - 1] - axis_x[0]) / (nx - 1).  Grid coordinates g = (p - origin) / voxel_size: centre i at g = i.
 *   ray      d_cam = ((u - K[0][2]) / K[0][0], (v - K[1][2]) / K[1][1], 1); d = R d_cam per row as (r0 dcx + r1 dcy) + r2;
 *            o = pose[:3, 3]; p(t) = o + t d, so t is camera z -- the convention of saf_frame.depth.  In grid coordinates
 *            g(t) = og + t gd with og = (o - origin) / voxel_size and gd = d / voxel_size, per axis.
 *            pose [4,4] camera->world and K [3,3] are DEVICE pointers as in saf_frame (no host synchronisation).  K must have no
 *            skew and a third row of (0, 0, 1); the call cannot read device memory, so it is the kernel that refuses any other K:
 *            every pixel is then a miss.
 *   range    t in [z_near, z_far] clipped by the slab method to 0 <= g <= n - 1 per axis (t1 = (0 - og) / gd, t2 = (n - 1 - og) / gd;
 *            an axis with gd = 0 keeps the range iff 0 <= og <= n - 1).  An empty range is a miss.
 *   samples  t_k = t_enter + k s, k = 0, 1, ... while t_k <= t_exit (at most 65536), s = (step_vox voxel_size) / max(|dx|, |dy|, |dz|).
 *   value    f_k = trilinear interpolation of tsdf at g(t_k): cell i = floor(g) clamped to [0, n - 2], offset g - i, per axis;
 *            a + f (b - a) along z, then y, then x.  The sample is OBSERVED iff all 8 corners have tsdf_weight > 0.
 *   hit      the first k with samples k and k + 1 both observed, f_k > 0 and f_{k+1} <= 0 (front faces only);
 *            t* = t_k + s (f_k / (f_k - f_{k+1})).
 *   out_depth [H,W] f32   t*, 0 for a miss (missing depth is 0, as in saf_frame.depth)
 *   out_voxel [H,W] i32   flat index (x ny + y) nz + z of the voxel nearest to g(t*) (round half to even per axis, clamped to the
 *                         grid), -1 for a miss
 *   out_rgb   [H,W,3] f32 (may be NULL) vol->rgb of that voxel; 0 for a miss or where the voxel's `weight` is 0
 * The volume needs at least 2 voxels per axis and fewer than 2^31 in all.  SAF_E_INVALID (on the host, nothing is launched) for a
 * NULL vol / pose / K / out_depth / out_voxel, non-positive sizes, step_vox <= 0 or z_far <= z_near.
 * One wave casts an 8 x 8-pixel tile; the corner taps are read as pairs along z (8-byte requests).
 */
int saf_raycast(const saf_volume* vol, const float* pose, const float* K, int32_t height, int32_t width, float step_vox,
                float z_near, float z_far, float* out_depth, int32_t* out_voxel, float* out_rgb, void* stream);

/*
 * dst[p, :] = src[index[p], :] for p = 0 .. n_index - 1, rows of zeros where index[p] < 0 (or >= n_src_rows): the rows of the
 * voxels a ray cast hit, for saf_query_scan (ABI 5).  Bytes are copied, whatever the dtype: row_bytes must be a multiple of 16
 * and src / dst 16-byte aligned (SAF_E_INVALID otherwise, as for NULL pointers and non-positive sizes; nothing is launched).
 */
int saf_gather_rows(const void* src, int64_t n_src_rows, int64_t row_bytes, const int32_t* index, int64_t n_index, void* dst,
                    void* stream);

/*
 * Per-object descriptors of a segmented volume (ABI 6; flood_fill_3d hands each object's {"clip_feats", "rgb", "voxels"} to the
 * in-situ classifier, handy_utils.py:400-404, and app_unity.py's /merge_objects, /rename_object and /memorize_objects work on
 * objects as wholes: this is the reduction of a voxel labelling to one row per object, on the device).
 *   slot       [N] i32: voxel n (flat index (x ny + y) nz + z) is a member of object k = slot[n] iff 0 <= k < n_objects; any other
 *              value means no object
 *   count      [K] i64 members of object k (K = n_objects);  bbox [K,6] i32 (xmin, ymin, zmin, xmax, ymax, zmax) and
 *              coord_sum [K,3] i64 over all members, in voxel indices.  An object without a member gets count 0, the box
 *              (nx, ny, nz, -1, -1, -1) and zeros elsewhere
 *   n_fused    [K] i64 and weight_sum [K] i64: the FUSED members (vol->weight > 0) and the sum of their weights
 *   rgb_mean   [K,3] f32 mean over the fused members of vol->rgb clamped to [0, 1] (the clamp of saf_sample_vertices)
 *   feat_mean  [K,D] f32 mean over the fused members of the normalised feature row (volume dtype f32 or bf16; SAF_F16 volumes: SAF_E_UNSUPPORTED; any feat_dim >= 1;
 *              rows on 16-byte boundaries are read 16 bytes per lane, others element by element); 0 where n_fused is 0
 *   normalize  SAF_NORM_L2 (f / |f|, NaN -> 0: a zero row contributes zeros and still counts in n_fused) or SAF_NORM_L2_CLAMP
 *              (f / max(|f|, 0.1)).  SAF_NORM_NONE returns SAF_E_UNSUPPORTED: raw rows have no bounded range, and the sums below
 *              are exact only for bounded terms
 *   workspace  saf_object_stats_workspace_bytes(n_voxels, n_objects, feat_dim) bytes, 256-byte aligned (0 for a bad size)
 * rgb_mean, feat_mean, weight_sum, n_fused and coord_sum may each be NULL; with feat_mean == NULL no feature row is read.  Every
 * output is written in full: the caller zeroes nothing.
 * Determinism: integer outputs are exact, and two calls on the same inputs return the same bytes in every output whatever the grid
 * or the scheduling.  The means are sums of rint(v 2^30) over terms v in [-1, 1] (a normalised element, a clamped colour; NaN
 * counts as 0, anything outside the range as its nearer end) held as 64-bit integers -- integer adds commute, and 2^31 members
 * times 2^30 stay below 2^63 --, finished as (double)S / (2^30 n_fused) and rounded once to f32.  The norm is the fp32 sum of
 * squares in a fixed order, sqrtf, and one IEEE division per element.
 * SAF_E_INVALID (on the host, nothing is launched) for a NULL vol / slot / count / bbox, n_objects < 1, a grid of 2^31 voxels or
 * more, a workspace that is too small or misaligned.
 * A wave walks fixed chunks of 512 voxels in raster order (objects are runs along z), accumulates consecutive members of one
 * object in registers and flushes them with 64-bit integer atomics when the slot changes or the chunk ends; `slot` and `weight`
 * are read once per voxel, feature rows only for fused members: 8 N + M (D s + 16) bytes for M fused members of s-byte elements.
 */
size_t saf_object_stats_workspace_bytes(int64_t n_voxels, int32_t n_objects, int32_t feat_dim);
int saf_object_stats(const saf_volume* vol, const int32_t* slot, int32_t n_objects, int32_t normalize, int64_t* count,
                     int64_t* n_fused, int64_t* weight_sum, int32_t* bbox /*[K,6]*/, int64_t* coord_sum /*[K,3]*/,
                     float* rgb_mean /*[K,3]*/, float* feat_mean /*[K,D]*/, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Overlap of two labellings of one lattice (added under ABI 7: additive, the version number stays; new capability: the reference
 * asks its in-situ classifier whether a newly found component "existed", handy_utils.py flood_fill_3d -- here the two versions of a
 * scan are compared voxel by voxel, and objects.assign_identities decides on the host which object is which).
 *   slot_a    [ax ay az] i32 and slot_b [bx by bz] i32: a dense object number per voxel, as for saf_object_stats (flat index
 *             (x ny + y) nz + z).  Voxel n is a member of object k = slot[n] iff 0 <= k < n_a (n_b); any other value means no object.
 *   mapping   the convention of saf_volume_carry: the two grids are boxes of one lattice, voxel (x, y, z) of `b` corresponds to
 *             voxel (x + off_x, y + off_y, z + off_z) of `a`; the caller passes off = b's index offset - a's.  The OVERLAP is the
 *             set of `b` voxels whose `a` voxel lies inside `a`.
 *   pair      [n_a, n_b] i64: pair[i, j] = overlap voxels that are members of i in `a` and of j in `b`
 *   in_a      [n_a] i64 members of i inside the overlap;  in_b [n_b] i64 likewise for `b`.  Members outside the overlap count
 *             nowhere.  pair.sum(1) <= in_a and pair.sum(0) <= in_b: the rest faces voxels without an object on the other side.
 *   workspace saf_object_overlap_workspace_bytes(n_a, n_b) bytes, 256-byte aligned (0 for a bad size): one (n_a + 1) x (n_b + 1)
 *             table of 64-bit counters, row n_a / column n_b standing for "no object"
 * Every output is written in full: the caller zeroes nothing.  An empty overlap gives zeros everywhere and SAF_OK.
 * Determinism: 64-bit integer atomics only -- the counts are exact, and two calls return the same bytes whatever the grid or the
 * scheduling.
 * SAF_E_INVALID (on the host, nothing is launched) for a NULL slot_a / slot_b / pair / in_a / in_b, non-positive sizes, a grid of
 * 2^31 voxels or more, n_a < 1 or n_b < 1, a workspace that is too small or not on a 256-byte boundary.  SAF_E_UNSUPPORTED for
 * n_a n_b > 2^24: the dense table would exceed 128 MB (the cap; scenes hold hundreds of objects).
 * Three launches (init, count, finish).  A wave takes 512 consecutive voxels of the flattened overlap box, z fastest; voxels that
 * are no member on either side are dropped by a ballot, and the wave issues ONE atomic per distinct pair key of the chunk (objects
 * are runs along z: a few as a rule), not one per voxel.  Both slots are read once per overlap voxel: 8 N_overlap bytes,
 * beside 24 (n_a + 1)(n_b + 1) for the table's init and finish.
 */
size_t saf_object_overlap_workspace_bytes(int32_t n_a, int32_t n_b);
int saf_object_overlap(const int32_t* slot_a, int32_t ax, int32_t ay, int32_t az, const int32_t* slot_b, int32_t bx, int32_t by,
                       int32_t bz, int32_t off_x, int32_t off_y, int32_t off_z, int32_t n_a, int32_t n_b, int64_t* pair /*[n_a,n_b]*/,
                       int64_t* in_a /*[n_a]*/, int64_t* in_b /*[n_b]*/, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Rig front-end (added under ABI 6: additive, the version number stays; magicleap2_camera_match.py states the problem and the
 * metadata layout, not this arithmetic -- its per-pixel loop has no occlusion test, its relative pose is not mirrored, and cv2's
 * fixed-point remap is not in the build image: parity with it is unpinned).  A headset frame has a depth and a colour image from
 * two cameras: two resolutions, two sets of intrinsics, a 5-coefficient lens distortion each, one pose each.  These calls take
 * such frames to the one pinhole K and one pose per frame that saf_frame assumes.  fp32 throughout, one IEEE operation at a time
 * in the order written here (tests/registration_reference.py restates it in NumPy).  The batch index b runs in the grid: one
 * launch covers a batch (batch <= 65535).
 *
 *   camera   a HOST struct, copied into the kernel arguments.  dist = (k1, k2, p1, p2, k3), OpenCV's order (the five entries of
 *            the headset's "Distortion"); no skew.  A "pinhole" camera below is one whose dist is IGNORED (taken as zeros).
 *            pixel -> ray: x = (u - cx) / fx;  ray -> pixel: u = fx x + cx (one product, one sum).
 *   D(x, y)  ideal -> distorted normalised coordinates:
 *              r2 = x x + y y;  rad = 1 + r2 (k1 + r2 (k2 + r2 k3))                        (innermost product first)
 *              tx = (2 p1) (x y) + p2 (r2 + 2 (x x));  ty = p1 (r2 + 2 (y y)) + (2 p2) (x y)
 *              xd = x rad + tx;  yd = y rad + ty
 *   D^-1     exactly 8 fixed-point steps from (x, y) = (xd, yd): x <- (xd - tx(x, y)) / rad(x, y), y <- (yd - ty(x, y)) / rad(x, y),
 *            both from the same (x, y).  The count is fixed so that the restatement can follow it.  rad <= 0 at any step, or a
 *            non-finite (x, y) after the last, makes the pixel MISSING.  With all-zero coefficients D and D^-1 are the identity,
 *            bit for bit.
 *   T_d2c    [B,4,4] f32 in DEVICE memory, row-major: depth-camera coordinates -> colour-camera coordinates of frame b
 *            (inv(pose_color) pose_depth for camera->world poses).  Q = R P + t per row as ((r0 Px + r1 Py) + r2 Pz) + t.
 *   depth    raw (distorted) images hold camera z, the convention of saf_frame.depth; a value is PRESENT iff it is finite and > 0
 *            (0, negative, NaN, +-inf are missing).
 *
 * saf_undistort_images: src [B,Hs,Ws,C] f32 channel-last (C = 3: rgb as the loaders yield it; C = 1: depth or label maps;
 *   1 <= C <= 4) seen by cam_src -> dst [B,Hd,Wd,C] as the pinhole cam_dst sees it.  Output pixel (u, v): (x, y) = its ray in
 *   cam_dst, (xd, yd) = D_src(x, y), (us, vs) = its pixel in cam_src.
 *     interp 0  nearest: (rint(us), rint(vs)), half to even; 0 outside the image
 *     interp 1  bilinear: cell (floor(us), floor(vs)), offsets us - floor(us), a + f (b - a) along u then along v; taps outside
 *               the image contribute 0
 *   Non-finite us / vs write 0.  Use nearest for depth and label maps: bilinear invents surfaces across depth edges and classes
 *   between labels (the Python layer does).
 *
 * saf_depth_to_color: depth [B,Hd,Wd] raw, seen by cam_depth -> out_depth [B,Hc,Wc] camera z in the pinhole cam_color, 0 where
 *   nothing lands.  A SCATTER: every present raw pixel (u, v) with depth z
 *     (x, y) = D_depth^-1 of its ray (missing: skipped);  P = (x z, y z, z);  Q = T_d2c[b] P; skipped unless Q.z is finite and > 0
 *     uc = fx_c (Q.x / Q.z) + cx_c, vc likewise (skipped unless finite)
 *     hx = min((0.5 (fx_c / fx_d)) (z / Q.z), max_footprint / 2) + 1/32, hy likewise with fy: half the depth pixel's size in
 *          colour pixels.  It ignores the rig's rotation and both lenses (a depth pixel at the rim of a strongly distorted image
 *          is larger than this says)
 *     it covers the integer colour pixels ceil(uc - hx) .. floor(uc + hx) x ceil(vc - hy) .. floor(vc + hy) inside the image
 *   and every covered pixel keeps the smallest Q.z.  The closed interval and the 1/32 make neighbouring footprints overlap rather
 *   than leave a gap; for an identity rig each pixel covers exactly itself even when uc is an ulp off an integer.  The minimum is an
 *   atomicMin on the bit pattern of Q.z as an unsigned integer (positive floats order as their bits: order-free, two calls return
 *   the same bytes) between a fill to +inf and a pass that writes 0 for +inf; the z-buffer is out_depth itself, so
 *   saf_depth_to_color_workspace_bytes returns 0 and workspace may be NULL (kept in the signature for a form that needs one).
 *   max_footprint: 1 .. 16 colour pixels (SAF_E_INVALID otherwise).  Why a splat and not a mesh of the depth image: a mesh
 *   bridges depth edges with triangles no camera saw, and needs an edge threshold to cut them; a footprint never spans two source
 *   pixels.  What it costs: a foreground edge is fattened by up to hx, and a magnification above max_footprint leaves gaps.
 *
 * saf_color_to_depth: the other direction (the reference script's).  A GATHER: output pixel (u, v) of the pinhole cam_depth_out
 *     z = the nearest sample of the raw depth through D_depth, exactly saf_undistort_images with interp = 0;
 *         out_depth[b,v,u] = z, 0 if missing
 *     P = (x z, y z, z) on the pinhole ray (x, y) of (u, v);  Q = T_d2c[b] P;  (xq, yq) = (Q.x / Q.z, Q.y / Q.z)
 *     (uc, vc) = the pixel of D_color(xq, yq) in cam_color; the raw colour image [B,Hc,Wc,3] is sampled there bilinearly (as
 *         interp 1): ONE interpolation of the raw image, not the reference's two
 *   VALID iff z is present, Q.z is finite and > 0, the cell lies inside the colour image (0 <= floor(uc) <= Wc - 2 and
 *   0 <= floor(vc) <= Hc - 2) and, with a zbuf, Q.z - zb <= occlusion_tol (metres), where zb = zbuf[b] at the nearest pixel
 *   (rint) of the pinhole projection (fx_z xq + cx_z, fy_z yq + cy_z); zb = 0 or a projection outside zbuf does not occlude.
 *   zbuf [B,Hz,Wz] is an out_depth of saf_depth_to_color for the pinhole cam_zbuf; zbuf == NULL disables the test (cam_zbuf is
 *   then not read).  out_rgb [B,Hd',Wd',3] is 0 where invalid; out_valid [B,Hd',Wd'] u8.
 *   D_color is a polynomial: far outside the colour camera's field of view it can fold a point back into the image.  The
 *   coefficients are taken to be valid over the depth camera's field of view; nothing here tests that.
 *
 * SAF_E_INVALID (on the host, nothing is launched) for NULL required pointers, non-positive sizes, a batch above 65535, channels
 * outside 1 .. 4, interp other than 0 / 1, or a camera whose fx / fy is not finite and positive.  Every index is tested on the
 * float before it is converted: any input (NaN, inf, 1e30, any T) stays in bounds.  One thread per source pixel (scatter) or
 * output pixel (gathers); a wave owns an 8 x 8-pixel tile, so that its taps share lines.
 */
typedef struct saf_camera {
  int32_t width, height;
  float fx, fy, cx, cy;
  float dist[5]; /* k1, k2, p1, p2, k3 */
} saf_camera;

int saf_undistort_images(const float* src, int32_t batch, int32_t channels, const saf_camera* cam_src, const saf_camera* cam_dst,
                         int32_t interp, float* dst, void* stream);
size_t saf_depth_to_color_workspace_bytes(int32_t batch, const saf_camera* cam_color);
int saf_depth_to_color(const float* depth, const saf_camera* cam_depth, const float* T_d2c /*[B,4,4]*/, int32_t batch,
                       const saf_camera* cam_color, int32_t max_footprint, float* out_depth, void* workspace,
                       size_t workspace_bytes, void* stream);
int saf_color_to_depth(const float* depth, const saf_camera* cam_depth, const saf_camera* cam_depth_out,
                       const float* T_d2c /*[B,4,4]*/, int32_t batch, const float* color, const saf_camera* cam_color,
                       const float* zbuf, const saf_camera* cam_zbuf, float occlusion_tol, float* out_depth, float* out_rgb,
                       uint8_t* out_valid, void* stream);

/*
 * Frame-to-model pose refinement (added under ABI 7: additive, the version number stays; nothing to mirror in the reference, which
 * fuses with the poses the capture app wrote).  A depth frame and a slightly wrong camera->world pose go in; the pose that puts the
 * frame's points on the zero set of the fused TSDF comes out, by a fixed Gauss-Newton on the device.  tests/pose_reference.py
 * restates everything below in NumPy.
 *
 * saf_pose_linearize -- residuals, Jacobian rows and the normal equations at one pose, over the pixel lattice
 * (u, v) = (stride i, stride j), i < ceil(width / stride), j < ceil(height / stride).  Per pixel, fp32, one IEEE operation at a
 * time in the order written here (grid, origin and voxel_size as in saf_raycast; pose [4,4], K [3,3] and depth [H,W] are DEVICE
 * pointers):
 *   point    z = depth[v][u]; the pixel is INVALID unless z > 0 and finite.  d_cam = ((u - K[0][2]) / K[0][0],
 *            (v - K[1][2]) / K[1][1], 1); q = (z dcx, z dcy, z); lever l_a = (R[a][0] q0 + R[a][1] q1) + R[a][2] q2;
 *            p_a = l_a + t_a; g_a = (p_a - origin_a) / voxel_size.  A K with skew or a third row other than (0, 0, 1) makes every
 *            pixel invalid (the call cannot read device memory).
 *   in-grid  invalid unless 0 <= g_a <= n_a - 1 on every axis (no extrapolation); cell i = floor(g) clamped to [0, n - 2],
 *            offset f = g - i, per axis; invalid unless all 8 corners have tsdf_weight > 0.
 *   residual r = trilinear tsdf at g: a + f (b - a) along z, then y, then x (c00, c01, c10, c11 -> c0, c1 -> r, first index x).
 *   gradient in voxel units from the same intermediates: d/dx = c1 - c0; d/dy = lerp(c01 - c00, c11 - c10, fx);
 *            d/dz = lerp(lerp(z00, z01, fy), lerp(z10, z11, fy), fx) with zxy the difference of the corner pair along z;
 *            n = grad / voxel_size (per metre; the TSDF is in units of trunc).
 *   band     invalid unless |r| < r_max (free space is saturated at +1 and carries no gradient).
 *   weight   w = 1 if |r| <= huber, else huber / |r|.
 *   row      J = (n, l x n), each cross-product component as (a b) - (c d): J3 = l1 n2 - l2 n1, J4 = l2 n0 - l0 n2,
 *            J5 = l0 n1 - l1 n0.  This is d r / d (v, omega) for the update R <- exp([omega]x) R, t <- t + v: a rotation about the
 *            camera centre.
 *   terms    in fp64 from these fp32 values: a_i = (double)w (double)J_i; a_i J_j for the 21 entries of the upper triangle
 *            (row-major: 00 01 .. 05 11 12 ..), a_i r for the 6 right-hand sides, ((double)w r) r for the cost, 1 for the count.
 *   out_system [32] f64 (device): slots 0..20 H = sum w J^T J, 21..26 b = sum w J r, 27 the cost, 28 n_valid, 29..31 zero.
 *   out_residual [H,W] f32 and out_jacobian [H,W,6] f32 (each may be NULL): r and J per pixel, NaN where the pixel is invalid or
 *            off the lattice.
 * Reduction: one wave owns an 8 x 8 tile of the lattice and adds its 64 pixels' terms in a butterfly over lane distances
 * 32, 16, .., 1; it writes one partial of 32 doubles per tile to the workspace.  One workgroup then adds the partials: thread
 * (g, k), g < 8, adds slot k of tiles g, g + 8, .. in that order, and the 8 group sums are added in the order of g.  No
 * floating-point atomics: the same inputs give the same bytes whatever the scheduling (the guarantee of saf_object_stats).
 *
 * saf_pose_refine -- the whole loop, enqueued back to back with no host synchronisation: for level l = 0 .. n_levels - 1,
 * iters[l] times: linearise at stride strides[l] at the current pose, then one workgroup
 *   1. adds the partials; K unsupported: status 4.  n_valid < min_valid: status 2;
 *   2. solves (H + damping diag(H) + 1e-12 I) xi = -b, xi = (v, omega), by Cholesky in fp64; a pivot that is not positive and
 *      finite: status 3;
 *   3. updates the pose, kept in fp64 in the workspace: R <- exp([omega]x) R (Rodrigues), t <- t + v;
 *   4. status 5 if the pose has left the input pose by more than max_shift_t (metres, |t - t_in|) or max_shift_r (radians, the
 *      angle of R R_in^T), or is not finite;
 *   5. writes the pose rounded to fp32 for the next linearisation and to pose_out, and appends the log record
 *      [stride, n_valid, cost / n_valid, |v|, |omega|, status of this step, 0, 0]  (status 0: |v| < tol_t and |omega| < tol_r;
 *      else 1; or the refusal 2 .. 5, then with the |v|, |omega| computed so far).
 * A level whose step converges ends there: its remaining iterations are skipped (their log rows stay zero) and the next level
 * begins; the last level's convergence ends the call with out_status 0.  All iterations used up: out_status 1, pose_out is the
 * last iterate.  On status 2, 3, 4 or 5 the call ends, a device flag makes the remaining launches return at once, and pose_out
 * is pose_in byte for byte.  out_log [sum(iters), 8] f64; rows never reached are zero.  pose_out [4,4] f32 (last row 0 0 0 1 on
 * status 0 / 1), out_status i32: all device memory, as is the workspace of saf_pose_workspace_bytes(height, width, smallest
 * stride) bytes, 256-byte aligned (0 for a non-positive size or stride).
 *
 * SAF_E_INVALID (on the host, nothing is launched) for NULL pointers (the two debug outputs excepted), non-positive sizes,
 * stride < 1, n_levels < 1, a level with fewer than 1 or more than 1000 iterations, huber or r_max not positive, another
 * parameter negative, a grid under 2 voxels per axis or of 2^31 voxels or more, a workspace that is small or misaligned.
 */
typedef struct saf_pose_params {
  float huber;       /* |r| up to which a residual has full weight (units of trunc) */
  float r_max;       /* residuals of this size or more are dropped (units of trunc; below 1: free space is +1) */
  float damping;     /* Levenberg factor on diag(H) */
  float tol_t;       /* metres */
  float tol_r;       /* radians */
  int32_t min_valid; /* fewer valid pixels than this: status 2 */
  float max_shift_t; /* metres */
  float max_shift_r; /* radians */
} saf_pose_params;

size_t saf_pose_workspace_bytes(int32_t height, int32_t width, int32_t min_stride);
int saf_pose_linearize(const saf_volume* vol, const float* depth, int32_t height, int32_t width, const float* pose, const float* K,
                       int32_t stride, float huber, float r_max, double* out_system /*[32]*/, float* out_residual /*[H,W]*/,
                       float* out_jacobian /*[H,W,6]*/, void* workspace, size_t workspace_bytes, void* stream);
int saf_pose_refine(const saf_volume* vol, const float* depth, int32_t height, int32_t width, const float* pose_in, const float* K,
                    const int32_t* strides, const int32_t* iters, int32_t n_levels, const saf_pose_params* params,
                    float* pose_out /*[4,4]*/, double* out_log /*[sum(iters),8]*/, int32_t* out_status, void* workspace,
                    size_t workspace_bytes, void* stream);

/*
 * Marching cubes on the TSDF, on the device: the mesh half of extract_mesh (clipfusion.py:723-739,
 * clip_seem_fusion.py:824-842) -- un-fused voxels (weight == 0) act as the reference's NaN mask, faces with a vertex on
 * an edge to an un-fused voxel are dropped, unused vertices never exist.  Two calls, because the sizes are results:
 *   count: classifies every cube; counts[0] = vertices, counts[1] = faces (device i64[2]; read them back to allocate);
 *   emit : verts [n_verts, 3] f32 in voxel-index coordinates (x, y, z) -- what skimage returns and the reference feeds
 *          to grid_sample / scales by voxel_size -- ordered by (owner voxel in raster order, axis); faces [n_faces, 3]
 *          i32 ordered by cube in raster order, normals toward positive tsdf.  Both calls take the same workspace
 *          (saf_marching_cubes_workspace_bytes, 256-byte aligned), untouched in between.
 * The triangulation of ambiguous cubes and the vertex order differ from scikit-image's Lewiner variant (not in the
 * build image: parity with it is unpinned); the vertex SET is one vertex per level-crossing grid edge in both.
 */
size_t saf_marching_cubes_workspace_bytes(int64_t n_voxels);
int saf_marching_cubes_count(const float* tsdf, const int32_t* weight, int32_t nx, int32_t ny, int32_t nz, float level,
                             void* workspace, size_t workspace_bytes, int64_t* counts, void* stream);
int saf_marching_cubes_emit(const float* tsdf, const int32_t* weight, int32_t nx, int32_t ny, int32_t nz, float level,
                            void* workspace, size_t workspace_bytes, float* verts, int64_t verts_capacity,
                            int32_t* faces, int64_t faces_capacity, void* stream);

/*
 * On-disk and wire formats of the fused results (host code, any thread).
 *   saf_save_npy   data (device memory when on_device != 0, read after `stream` has drained; else host memory) ->
 *                  NumPy .npy v1.0 at `path`, C order.  dtype_code: 0 f32, 1 bf16 (written as 2-byte records '<V2'),
 *                  2 f16, 3 i32, 4 i64, 5 u8.  Device arrays stream through two pinned 64 MiB buffers (copy of chunk
 *                  k + 1 beside the write of chunk k).  The files of save_files_and_broadcast (clip_seem_fusion.py:563-581).
 *   saf_mesh_json  {"vertices": [[x, y, z], ...], "faces": [[i, j, k], ...], "colors": [[...], ...]} (clip_seem_fusion.py:
 *                  553-559, handy_utils.py:233-239) from HOST arrays; floats are printed as the shortest decimal that
 *                  round-trips the double value of each f32, so a JSON parser returns exactly ndarray.tolist().
 *                  *out is malloc'ed: release it with saf_free.
 *   saf_save_ply   binary little-endian PLY (x y z float, optional red green blue alpha uchar from colours in 0..1,
 *                  faces as `list uchar int`) from HOST arrays: mesh_rgb.ply / mesh_segmentation.ply (:584-600).
 */
int saf_save_npy(const void* data, int32_t on_device, int32_t dtype_code, const int64_t* shape, int32_t ndim,
                 const char* path, void* stream);
int saf_mesh_json(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* colors,
                  int32_t n_color, char** out, int64_t* out_len);
/* A HOST array [rows, cols] (cols == 0: flat) as the JSON text of ndarray.tolist(), Python's separators; dtype_code 0 f32, 3 i32,
 * 4 i64, 6 f64.  The voxel lists and per-object meshes of scene_knowledge.json (clip_seem_fusion.py:393-417, :603-604). */
int saf_array_json(const void* data, int32_t dtype_code, int64_t rows, int32_t cols, char** out, int64_t* out_len);
void saf_free(void* p);
int saf_save_ply(const char* path, const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                 const float* colors, int32_t n_color);

/* Per-voxel argmax of the label histogram with the all-zero row -> -1 rule
 * (clip_seem_fusion.py:315-325).  out[N] i32. */
int saf_label_argmax(const int32_t* labels_one_hot, int64_t n_voxels, int32_t n_classes,
                     int32_t* out, void* stream);

/* ---- the connected-component core of flood_fill_3d (handy_utils.py:295-480) ----
 * labels [nx,ny,nz] i32 class ids (row-major, z fastest), as produced by saf_label_argmax reshaped to the
 * grid (clip_seem_fusion.py:322-338).  Voxels of `null_class` (133 in the reference, handy_utils.py:383)
 * and empty voxels (-1) belong to no object.  Objects are the 26-connected sets of equal class
 * (handy_utils.py:312-344); objects of fewer than `min_voxels` voxels are rejected (3 in the reference,
 * :390).  The k-th accepted object in raster order of its first voxel gets the index -2 - k
 * (handy_utils.py:352-353, :447-450 without a trained in-situ model):
 *   obj_ids   [N] i32   -1 or -2 - k                      (= the reference's voxel_obj_ids)
 *   n_objects [1] i32   number of accepted objects
 *   obj_first / obj_class / obj_count [max_objects] i32 (each may be NULL): first voxel (flat index),
 *   class id and voxel count of object k, for k < max_objects. */
size_t saf_label_components_workspace_bytes(int64_t n_voxels);
int saf_label_components(const int32_t* labels, int32_t nx, int32_t ny, int32_t nz, int32_t null_class,
                         int32_t min_voxels, int32_t* obj_ids, int32_t* n_objects, int32_t max_objects,
                         int32_t* obj_first, int32_t* obj_class, int32_t* obj_count, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAF_H */
