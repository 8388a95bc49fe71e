// saf_track.hip -- refining a camera pose against the fused TSDF on gfx950 (new capability: the reference fuses with the poses the
// capture app wrote; a headset's poses drift by a voxel or two over a scan):
//   * pose_linearize_kernel : one depth pixel of the sampled lattice per lane, one 8 x 8 lattice tile per wave -- the point-to-TSDF
//                             residual, its 6-vector Jacobian row and the pixel's terms of the normal equations, reduced over the
//                             wave in a fixed lane pattern into one partial of 32 doubles per tile;
//   * pose_sum_kernel       : the tile partials summed in a fixed order (saf_pose_linearize's out_system);
//   * pose_init_kernel / pose_solve_kernel : the Gauss-Newton loop of saf_pose_refine -- the same sum, a damped 6 x 6 Cholesky solve
//                             in fp64, the pose update and the stopping rules, all decided on the device.
//
// Numerics contract (include/saf.h, saf_pose_linearize; tests/pose_reference.py restates it in NumPy): the residual is the ray
// cast's reading of the TSDF as a field, whose one C statement is saf_field_dev.h (the grid frame, the pixel's ray, the trilinear
// sample and its intermediates); the rest of the per-pixel chain is below, every fp32 operation written on its own, in the order
// stated there; the translation unit is compiled with -ffp-contract=off and divisions are IEEE.  No floating-point atomics
// anywhere: the same inputs give the same bytes whatever the scheduling.
#include <math.h>

#include "saf_field_dev.h"

#pragma clang fp contract(off)

namespace saf {
namespace {

constexpr int kLinThreads = 256;  // four waves: a 16 x 16 block of the lattice, one 8 x 8 tile per wave
constexpr int kSysSlots = 32;     // doubles per partial: H (21), b (6), cost, n_valid, 3 x zero
constexpr int kSysUsed = 29;
constexpr int kSumThreads = 256;  // 8 groups of 32 slots
constexpr size_t kStateBytes = 512;

// What the iterations of one saf_pose_refine call share (the head of its workspace).
struct PoseState {
  double R[9], t[3];    // the current iterate, camera->world
  double R0[9], t0[3];  // the input pose
  float pose32[16];     // the current iterate as the next linearisation reads it
  float pose_in[16];    // the input pose, byte for byte
  int done;             // the call has finished: the remaining launches return at once
  int level_done;       // levels up to this one have converged: their remaining launches return at once
};
static_assert(sizeof(PoseState) <= kStateBytes, "PoseState outgrew its slot");

struct LinArgs {
  FieldArgs field;
  const float* depth;
  const float* pose;
  const float* K;
  const PoseState* state;  // NULL for saf_pose_linearize
  double* partials;
  float* out_residual;
  float* out_jacobian;
  int height, width;
  int stride, lat_w, lat_h, tiles_x, tiles_y;
  int level;
  float huber, r_max;
};

__device__ __forceinline__ double wave_sum(double x) {
  // fixed pattern: lane i ends with the sum over all 64 lanes, added in the order of a butterfly over lane distance 32, 16, ..., 1
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
  return x;
}

__global__ __launch_bounds__(kLinThreads) void pose_linearize_kernel(const LinArgs A) {
  if (A.state && (A.state->done || A.state->level_done >= A.level)) return;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int bx = (int)blockIdx.x % ((A.tiles_x + 1) / 2), by = (int)blockIdx.x / ((A.tiles_x + 1) / 2);
  const int tx = bx * 2 + (wave & 1), ty = by * 2 + (wave >> 1);
  if (tx >= A.tiles_x || ty >= A.tiles_y) return;  // (the whole wave)
  const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
  const bool on_lattice = i < A.lat_w && j < A.lat_h;
  const int u = on_lattice ? i * A.stride : 0, v = on_lattice ? j * A.stride : 0;  // < width, < height
  const int64_t pix = (int64_t)v * A.width + u;

  const FieldArgs& F = A.field;
  const GridFrame G = grid_frame(F);
  const float vs = G.vs;
  const float* P = A.pose;

  const float z = A.depth[pix];
  bool ok = on_lattice && z > 0.0f && z <= 3.402823466e38f;  // (NaN fails both)
  ok = ok && is_pinhole(A.K);
  // the point: q = z d_cam, lever l = R q, p = l + t
  float dcx, dcy;
  pixel_ray(A.K, u, v, dcx, dcy);
  const float q0 = z * dcx, q1 = z * dcy, q2 = z;
  const float l0 = (P[0] * q0 + P[1] * q1) + P[2] * q2;
  const float l1 = (P[4] * q0 + P[5] * q1) + P[6] * q2;
  const float l2 = (P[8] * q0 + P[9] * q1) + P[10] * q2;
  const float p0 = l0 + P[3], p1 = l1 + P[7], p2 = l2 + P[11];
  const float gx = (p0 - G.ox) / vs, gy = (p1 - G.oy) / vs, gz = (p2 - G.oz) / vs;
  ok = ok && gx >= 0.0f && gx <= (float)(F.nx - 1) && gy >= 0.0f && gy <= (float)(F.ny - 1) && gz >= 0.0f &&
       gz <= (float)(F.nz - 1);

  float r = 0.0f, w = 0.0f;
  float J0 = 0.0f, J1 = 0.0f, J2 = 0.0f, J3 = 0.0f, J4 = 0.0f, J5 = 0.0f;
  if (ok) {  // (only then are the grid coordinates known to be finite and inside the grid)
    // the residual: trilinear, z then y then x
    const FieldSample f = sample_field(F, gx, gy, gz);
    ok = f.observed;
    r = f.value;
    // its gradient in voxel units, from the same intermediates
    const float ddx = f.c1 - f.c0;
    const float ddy = lerp(f.c01 - f.c00, f.c11 - f.c10, f.fx);
    const float dz0 = lerp(f.t00.b - f.t00.a, f.t01.b - f.t01.a, f.fy);
    const float dz1 = lerp(f.t10.b - f.t10.a, f.t11.b - f.t11.a, f.fy);
    const float ddz = lerp(dz0, dz1, f.fx);
    const float n0 = ddx / vs, n1 = ddy / vs, n2 = ddz / vs;
    const float ar = __builtin_fabsf(r);
    ok = ok && ar < A.r_max;
    w = ar <= A.huber ? 1.0f : A.huber / ar;
    J0 = n0;
    J1 = n1;
    J2 = n2;
    {
      const float a = l1 * n2, b = l2 * n1;
      J3 = a - b;
    }
    {
      const float a = l2 * n0, b = l0 * n2;
      J4 = a - b;
    }
    {
      const float a = l0 * n1, b = l1 * n0;
      J5 = a - b;
    }
  }

  if (on_lattice) {
    const float nanv = __builtin_nanf("");
    if (A.out_residual) A.out_residual[pix] = ok ? r : nanv;
    if (A.out_jacobian) {
      float* o = A.out_jacobian + 6 * pix;
      o[0] = ok ? J0 : nanv;
      o[1] = ok ? J1 : nanv;
      o[2] = ok ? J2 : nanv;
      o[3] = ok ? J3 : nanv;
      o[4] = ok ? J4 : nanv;
      o[5] = ok ? J5 : nanv;
    }
  }

  // the pixel's terms in fp64 from the fp32 values; an invalid pixel contributes exact zeros
  const double wd = ok ? (double)w : 0.0, rd = ok ? (double)r : 0.0;
  const double j0 = ok ? (double)J0 : 0.0, j1 = ok ? (double)J1 : 0.0, j2 = ok ? (double)J2 : 0.0;
  const double j3 = ok ? (double)J3 : 0.0, j4 = ok ? (double)J4 : 0.0, j5 = ok ? (double)J5 : 0.0;
  const double a0 = wd * j0, a1 = wd * j1, a2 = wd * j2, a3 = wd * j3, a4 = wd * j4, a5 = wd * j5;
  double* out = A.partials + (int64_t)(ty * A.tiles_x + tx) * kSysSlots;
  double s;
#define SAF_SLOT(k, expr)          \
  s = wave_sum(expr);              \
  if (lane == ((k) & 63)) out[k] = s;
  SAF_SLOT(0, a0 * j0)
  SAF_SLOT(1, a0 * j1)
  SAF_SLOT(2, a0 * j2)
  SAF_SLOT(3, a0 * j3)
  SAF_SLOT(4, a0 * j4)
  SAF_SLOT(5, a0 * j5)
  SAF_SLOT(6, a1 * j1)
  SAF_SLOT(7, a1 * j2)
  SAF_SLOT(8, a1 * j3)
  SAF_SLOT(9, a1 * j4)
  SAF_SLOT(10, a1 * j5)
  SAF_SLOT(11, a2 * j2)
  SAF_SLOT(12, a2 * j3)
  SAF_SLOT(13, a2 * j4)
  SAF_SLOT(14, a2 * j5)
  SAF_SLOT(15, a3 * j3)
  SAF_SLOT(16, a3 * j4)
  SAF_SLOT(17, a3 * j5)
  SAF_SLOT(18, a4 * j4)
  SAF_SLOT(19, a4 * j5)
  SAF_SLOT(20, a5 * j5)
  SAF_SLOT(21, a0 * rd)
  SAF_SLOT(22, a1 * rd)
  SAF_SLOT(23, a2 * rd)
  SAF_SLOT(24, a3 * rd)
  SAF_SLOT(25, a4 * rd)
  SAF_SLOT(26, a5 * rd)
  SAF_SLOT(27, (wd * rd) * rd)
  SAF_SLOT(28, ok ? 1.0 : 0.0)
#undef SAF_SLOT
  if (lane >= kSysUsed && lane < kSysSlots) out[lane] = 0.0;
}

__global__ __launch_bounds__(256) void pose_fill_nan_kernel(float* __restrict__ dst, int64_t n) {
  const float nanv = __builtin_nanf("");
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = nanv;
}

// The partials of n_tiles tiles summed in a fixed order by one workgroup of kSumThreads: thread (g, k) adds slot k of the tiles
// g, g + 8, g + 16, ... in that order, and thread (0, k) then adds the 8 group sums in the order of g.  total[] is in LDS.
__device__ __forceinline__ void sum_partials(const double* __restrict__ partials, int n_tiles, double (*group)[kSysSlots],
                                             double* total) {
  const int k = (int)threadIdx.x & (kSysSlots - 1), g = (int)threadIdx.x / kSysSlots;
  constexpr int kGroups = kSumThreads / kSysSlots;
  double s = 0.0;
  for (int t = g; t < n_tiles; t += kGroups) s = s + partials[(int64_t)t * kSysSlots + k];
  group[g][k] = s;
  __syncthreads();
  if (g == 0) {
    double a = group[0][k];
    for (int q = 1; q < kGroups; ++q) a = a + group[q][k];
    total[k] = a;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kSumThreads) void pose_sum_kernel(const double* __restrict__ partials, int n_tiles,
                                                               double* __restrict__ out_system) {
  __shared__ double group[kSumThreads / kSysSlots][kSysSlots];
  __shared__ double total[kSysSlots];
  sum_partials(partials, n_tiles, group, total);
  if (threadIdx.x < kSysSlots) out_system[threadIdx.x] = total[threadIdx.x];
}

struct SolveArgs {
  PoseState* state;
  const double* partials;
  const float* K;
  float* pose_out;
  double* out_log;  // this iteration's row
  int* out_status;
  int n_tiles, stride, level, last_level;
  saf_pose_params prm;
};

__global__ __launch_bounds__(64) void pose_init_kernel(PoseState* st, const float* __restrict__ pose_in, float* __restrict__ pose_out,
                                                        double* __restrict__ out_log, int log_doubles, int* __restrict__ out_status) {
  const int t = (int)threadIdx.x;
  for (int i = t; i < log_doubles; i += 64) out_log[i] = 0.0;
  if (t < 16) {
    const float x = pose_in[t];
    st->pose32[t] = x;
    st->pose_in[t] = x;
    pose_out[t] = x;
    const int row = t >> 2, col = t & 3;
    if (row < 3) {
      if (col < 3) {
        st->R[row * 3 + col] = (double)x;
        st->R0[row * 3 + col] = (double)x;
      } else {
        st->t[row] = (double)x;
        st->t0[row] = (double)x;
      }
    }
  }
  if (t == 0) {
    st->done = 0;
    st->level_done = -1;
    *out_status = 1;
  }
}

// One Gauss-Newton step.  The 6 x 6 system lives in LDS (a dynamically indexed private array would land in scratch memory).
__global__ __launch_bounds__(kSumThreads) void pose_solve_kernel(const SolveArgs A) {
  PoseState* st = A.state;
  if (st->done || st->level_done >= A.level) return;
  __shared__ double group[kSumThreads / kSysSlots][kSysSlots];
  __shared__ double total[kSysSlots];
  __shared__ double M[6][6];
  __shared__ double x[6];
  __shared__ double E[9], Rn[9];
  sum_partials(A.partials, A.n_tiles, group, total);
  if (threadIdx.x != 0) return;

  const saf_pose_params& prm = A.prm;
  const double n_valid = total[28];
  const double mean_cost = n_valid > 0.0 ? total[27] / n_valid : 0.0;
  int status = 1;
  double step_t = 0.0, step_r = 0.0;
  if (!is_pinhole(A.K)) {
    status = 4;
  } else if (n_valid < (double)prm.min_valid) {
    status = 2;
  } else {
    // (H + damping diag(H) + 1e-12 I) xi = -b by Cholesky, H from the upper triangle
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) {
        M[i][j] = total[k];
        M[j][i] = total[k];
        ++k;
      }
    for (int i = 0; i < 6; ++i) {
      M[i][i] = (M[i][i] + (double)prm.damping * M[i][i]) + 1e-12;
      x[i] = -total[21 + i];
    }
    bool pd = true;
    for (int j = 0; j < 6 && pd; ++j) {
      double d = M[j][j];
      for (int q = 0; q < j; ++q) d = d - M[j][q] * M[j][q];
      if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) {
        pd = false;
        break;
      }
      const double ljj = sqrt(d);
      M[j][j] = ljj;
      for (int i = j + 1; i < 6; ++i) {
        double s = M[i][j];
        for (int q = 0; q < j; ++q) s = s - M[i][q] * M[j][q];
        M[i][j] = s / ljj;
      }
    }
    if (!pd) {
      status = 3;
    } else {
      for (int i = 0; i < 6; ++i) {  // L y = -b
        double s = x[i];
        for (int q = 0; q < i; ++q) s = s - M[i][q] * x[q];
        x[i] = s / M[i][i];
      }
      for (int i = 5; i >= 0; --i) {  // L^T xi = y
        double s = x[i];
        for (int q = i + 1; q < 6; ++q) s = s - M[q][i] * x[q];
        x[i] = s / M[i][i];
      }
      const double v0 = x[0], v1 = x[1], v2 = x[2], w0 = x[3], w1 = x[4], w2 = x[5];
      step_t = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
      const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
      step_r = sqrt(th2);
      // exp([omega]x) = I + a [omega]x + b [omega]x^2 (Rodrigues); the series below 1e-4 rad, where it is exact to fp64
      double a, b;
      if (step_r < 1e-4) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
      } else {
        a = sin(step_r) / step_r;
        b = (1.0 - cos(step_r)) / th2;
      }
      E[0] = 1.0 - b * (w1 * w1 + w2 * w2);
      E[1] = b * (w0 * w1) - a * w2;
      E[2] = b * (w0 * w2) + a * w1;
      E[3] = b * (w0 * w1) + a * w2;
      E[4] = 1.0 - b * (w0 * w0 + w2 * w2);
      E[5] = b * (w1 * w2) - a * w0;
      E[6] = b * (w0 * w2) - a * w1;
      E[7] = b * (w1 * w2) + a * w0;
      E[8] = 1.0 - b * (w0 * w0 + w1 * w1);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = (E[i * 3] * st->R[j] + E[i * 3 + 1] * st->R[3 + j]) + E[i * 3 + 2] * st->R[6 + j];
      for (int i = 0; i < 9; ++i) st->R[i] = Rn[i];
      st->t[0] = st->t[0] + v0;
      st->t[1] = st->t[1] + v1;
      st->t[2] = st->t[2] + v2;
      // the total departure from the input pose: |t - t0| and the angle of R R0^T
      const double d0 = st->t[0] - st->t0[0], d1 = st->t[1] - st->t0[1], d2 = st->t[2] - st->t0[2];
      const double shift_t = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          E[i * 3 + j] = (st->R[i * 3] * st->R0[j * 3] + st->R[i * 3 + 1] * st->R0[j * 3 + 1]) + st->R[i * 3 + 2] * st->R0[j * 3 + 2];
      const double s0 = E[7] - E[5], s1 = E[2] - E[6], s2 = E[3] - E[1];
      const double sn = 0.5 * sqrt((s0 * s0 + s1 * s1) + s2 * s2);
      const double cs = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
      const double shift_r = atan2(sn, cs);
      const bool finite = shift_t <= 1.7976931348623157e308 && shift_r <= 1.7976931348623157e308;  // (NaN fails)
      if (!finite || shift_t > (double)prm.max_shift_t || shift_r > (double)prm.max_shift_r)
        status = 5;
      else if (step_t < (double)prm.tol_t && step_r < (double)prm.tol_r)
        status = 0;
    }
  }

  double* log = A.out_log;
  log[0] = (double)A.stride;
  log[1] = n_valid;
  log[2] = mean_cost;
  log[3] = step_t;
  log[4] = step_r;
  log[5] = (double)status;
  log[6] = 0.0;
  log[7] = 0.0;

  if (status >= 2) {  // refused: the input pose comes back byte for byte
    for (int i = 0; i < 16; ++i) A.pose_out[i] = st->pose_in[i];
    *A.out_status = status;
    st->done = 1;
    return;
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) st->pose32[i * 4 + j] = (float)st->R[i * 3 + j];
    st->pose32[i * 4 + 3] = (float)st->t[i];
  }
  st->pose32[12] = 0.0f;
  st->pose32[13] = 0.0f;
  st->pose32[14] = 0.0f;
  st->pose32[15] = 1.0f;
  for (int i = 0; i < 16; ++i) A.pose_out[i] = st->pose32[i];
  if (status == 0) {
    st->level_done = A.level;  // the rest of this level is skipped; the last level's convergence is the call's
    if (A.last_level) st->done = 1;
  }
  *A.out_status = (status == 0 && A.last_level) ? 0 : 1;
}

inline int lattice(int n, int stride) { return (int)(((int64_t)n + stride - 1) / stride); }
inline int64_t tiles_of(int height, int width, int stride) {
  return (int64_t)((lattice(width, stride) + 7) / 8) * ((lattice(height, stride) + 7) / 8);
}

int check_common(const char* what, const saf_volume* vol, const float* depth, int height, int width, const float* pose, const float* K) {
  if (!vol || !depth || !pose || !K || height <= 0 || width <= 0)
    return fail(SAF_E_INVALID, "%s: bad arguments (%d x %d pixels; vol, depth, pose and K must not be NULL)", what, (int)height, (int)width);
  if (int rc = check_field_volume(what, vol)) return rc;
  return check_pixel_count(what, height, width);
}

void fill_lin_args(LinArgs& a, const saf_volume* vol, const float* depth, int height, int width, const float* pose, const float* K,
                   int stride, float huber, float r_max, void* workspace) {
  a.field = field_args(vol);
  a.depth = depth;
  a.pose = pose;
  a.K = K;
  a.state = nullptr;
  a.partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + kStateBytes);
  a.out_residual = nullptr;
  a.out_jacobian = nullptr;
  a.height = height;
  a.width = width;
  a.stride = stride;
  a.lat_w = lattice(width, stride);
  a.lat_h = lattice(height, stride);
  a.tiles_x = (a.lat_w + 7) / 8;
  a.tiles_y = (a.lat_h + 7) / 8;
  a.level = 0;
  a.huber = huber;
  a.r_max = r_max;
}

inline unsigned lin_blocks(const LinArgs& a) { return (unsigned)(((a.tiles_x + 1) / 2) * ((a.tiles_y + 1) / 2)); }

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" {

size_t saf_pose_workspace_bytes(int32_t height, int32_t width, int32_t min_stride) {
  if (height <= 0 || width <= 0 || min_stride < 1 || (int64_t)height * width > 0x7fffffff) return 0;
  return kStateBytes + (size_t)tiles_of(height, width, min_stride) * kSysSlots * sizeof(double);
}

int saf_pose_linearize(const saf_volume* vol, const float* depth, int32_t height, int32_t width, const float* pose, const float* K,
                       int32_t stride, float huber, float r_max, double* out_system, float* out_residual, float* out_jacobian,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_common("pose linearize", vol, depth, height, width, pose, K)) return rc;
  if (stride < 1 || !out_system || !(huber > 0.0f) || !(r_max > 0.0f))
    return fail(SAF_E_INVALID, "pose linearize: bad arguments (stride = %d, huber = %g, r_max = %g, out_system %s)", (int)stride,
                (double)huber, (double)r_max, out_system ? "given" : "NULL");
  if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < saf_pose_workspace_bytes(height, width, stride))
    return fail(SAF_E_INVALID, "pose linearize: the workspace is NULL, not 256-byte aligned or smaller than the %zu bytes of "
                "saf_pose_workspace_bytes", saf_pose_workspace_bytes(height, width, stride));
  hipStream_t s = static_cast<hipStream_t>(stream);
  LinArgs a;
  fill_lin_args(a, vol, depth, height, width, pose, K, stride, huber, r_max, workspace);
  a.out_residual = out_residual;
  a.out_jacobian = out_jacobian;
  const int64_t npix = (int64_t)height * width;
  if (out_residual) hipLaunchKernelGGL(pose_fill_nan_kernel, dim3(grid_1d(npix, 16)), dim3(256), 0, s, out_residual, npix);
  if (out_jacobian) hipLaunchKernelGGL(pose_fill_nan_kernel, dim3(grid_1d(6 * npix, 16)), dim3(256), 0, s, out_jacobian, 6 * npix);
  hipLaunchKernelGGL(pose_linearize_kernel, dim3(lin_blocks(a)), dim3(kLinThreads), 0, s, a);
  hipLaunchKernelGGL(pose_sum_kernel, dim3(1), dim3(kSumThreads), 0, s, a.partials, a.tiles_x * a.tiles_y, out_system);
  return check_launch("pose_linearize_kernel");
}

int saf_pose_refine(const saf_volume* vol, const float* depth, int32_t height, int32_t width, const float* pose_in, const float* K,
                    const int32_t* strides, const int32_t* iters, int32_t n_levels, const saf_pose_params* params, float* pose_out,
                    double* out_log, int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_common("pose refine", vol, depth, height, width, pose_in, K)) return rc;
  if (!strides || !iters || n_levels < 1 || !params || !pose_out || !out_log || !out_status)
    return fail(SAF_E_INVALID, "pose refine: bad arguments (%d levels; strides, iters, params, pose_out, out_log and out_status must "
                "not be NULL)", (int)n_levels);
  int min_stride = 0x7fffffff;
  int64_t total_iters = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (strides[l] < 1 || iters[l] < 1 || iters[l] > 1000)
      return fail(SAF_E_INVALID, "pose refine: level %d has stride %d and %d iterations (stride >= 1, 1 to 1000 iterations)", l,
                  (int)strides[l], (int)iters[l]);
    min_stride = strides[l] < min_stride ? strides[l] : min_stride;
    total_iters += iters[l];
  }
  if (!(params->huber > 0.0f) || !(params->r_max > 0.0f) || !(params->damping >= 0.0f) || !(params->tol_t >= 0.0f) ||
      !(params->tol_r >= 0.0f) || !(params->max_shift_t >= 0.0f) || !(params->max_shift_r >= 0.0f))
    return fail(SAF_E_INVALID, "pose refine: bad parameters (huber = %g and r_max = %g must be positive, the others not negative)",
                (double)params->huber, (double)params->r_max);
  if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < saf_pose_workspace_bytes(height, width, min_stride))
    return fail(SAF_E_INVALID, "pose refine: the workspace is NULL, not 256-byte aligned or smaller than the %zu bytes of "
                "saf_pose_workspace_bytes", saf_pose_workspace_bytes(height, width, min_stride));
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoseState* st = static_cast<PoseState*>(workspace);
  hipLaunchKernelGGL(pose_init_kernel, dim3(1), dim3(64), 0, s, st, pose_in, pose_out, out_log, (int)(total_iters * 8), out_status);
  int row = 0;
  for (int l = 0; l < n_levels; ++l) {
    LinArgs a;
    fill_lin_args(a, vol, depth, height, width, st->pose32, K, strides[l], params->huber, params->r_max, workspace);
    a.state = st;
    a.level = l;
    SolveArgs b;
    b.state = st;
    b.partials = a.partials;
    b.K = K;
    b.pose_out = pose_out;
    b.out_status = out_status;
    b.n_tiles = a.tiles_x * a.tiles_y;
    b.stride = strides[l];
    b.level = l;
    b.last_level = l == n_levels - 1;
    b.prm = *params;
    for (int it = 0; it < iters[l]; ++it, ++row) {
      b.out_log = out_log + (int64_t)row * 8;
      hipLaunchKernelGGL(pose_linearize_kernel, dim3(lin_blocks(a)), dim3(kLinThreads), 0, s, a);
      hipLaunchKernelGGL(pose_solve_kernel, dim3(1), dim3(kSumThreads), 0, s, b);
    }
  }
  return check_launch("pose_solve_kernel");
}

}  // extern "C"
