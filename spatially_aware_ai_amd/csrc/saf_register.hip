// saf_register.hip -- the rig front-end on gfx950: a headset's depth and colour cameras (two resolutions, two sets of intrinsics,
// a 5-coefficient lens distortion each, one pose each -- the captures magicleap2_camera_match.py prepares) brought to the one
// pinhole K and one pose per frame that saf_frame, integrate() and backproject_pcd assume:
//   * undistort_kernel      : a raw image resampled into a pinhole camera (nearest or bilinear), any 1 .. 4 channels;
//   * splat_kernel          : raw depth -> the pinhole colour camera, one thread per SOURCE pixel, a footprint of colour pixels
//                             per depth pixel, z-buffered with atomicMin on the bit pattern of the positive camera z
//                             (fill_kernel before it, finish_kernel after it);
//   * color_to_depth_kernel : per pixel of the pinhole depth camera the depth (nearest) and the colour the colour camera saw of
//                             that point (one bilinear tap of the RAW colour image), with an occlusion test against a splat.
//
// Numerics contract (include/saf.h, "Rig front-end"; tests/registration_reference.py restates it in NumPy): every fp32 operation
// below is written on its own, in the order stated there; the translation unit is compiled with -ffp-contract=off and divisions
// are IEEE.  Every index is tested on the float before it is converted, so any input (NaN, inf, 1e30, any T) stays in bounds.
#include <math.h>

#include "saf_field_dev.h"  // lerp

#pragma clang fp contract(off)

namespace saf {
namespace {

constexpr int kRegThreads = 256;  // four waves: a 16 x 16-pixel block, one 8 x 8 tile per wave (as saf_raycast.hip)
constexpr int kRegBlock = 16;
constexpr unsigned kInfBits = 0x7f800000u;
constexpr int kInverseSteps = 8;

// saf_camera by value: scalars only, so that it stays in (scalar) registers
struct Cam {
  int w, h;
  float fx, fy, cx, cy;
  float k1, k2, p1, p2, k3;
};

__device__ __forceinline__ bool tile_pixel(int w, int h, int& u, int& v) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  u = (int)blockIdx.x * kRegBlock + (wave & 1) * 8 + (lane & 7);
  v = (int)blockIdx.y * kRegBlock + (wave >> 1) * 8 + (lane >> 3);
  return u < w && v < h;
}

__device__ __forceinline__ bool finite(float x) { return __builtin_fabsf(x) < INFINITY; }  // false for NaN

// the radial factor and the tangential terms of the lens at normalised (x, y)
__device__ __forceinline__ void lens_terms(const Cam& c, float x, float y, float& rad, float& tx, float& ty) {
  const float xx = x * x;
  const float yy = y * y;
  const float r2 = xx + yy;
  const float a = r2 * c.k3;
  const float b = c.k2 + a;
  const float cc = r2 * b;
  const float d = c.k1 + cc;
  const float e = r2 * d;
  rad = 1.0f + e;
  const float xy = x * y;
  const float p1xy = (2.0f * c.p1) * xy;
  const float p2xy = (2.0f * c.p2) * xy;
  const float gx = r2 + 2.0f * xx;
  const float gy = r2 + 2.0f * yy;
  const float p2gx = c.p2 * gx;
  const float p1gy = c.p1 * gy;
  tx = p1xy + p2gx;
  ty = p1gy + p2xy;
}

// D: ideal -> distorted
__device__ __forceinline__ void distort(const Cam& c, float x, float y, float& xd, float& yd) {
  float rad, tx, ty;
  lens_terms(c, x, y, rad, tx, ty);
  const float xr = x * rad;
  const float yr = y * rad;
  xd = xr + tx;
  yd = yr + ty;
}

// D^-1: exactly kInverseSteps fixed-point steps from (xd, yd); false = missing
__device__ __forceinline__ bool undistort_point(const Cam& c, float xd, float yd, float& x, float& y) {
  x = xd;
  y = yd;
  bool ok = true;
#pragma unroll 1
  for (int i = 0; i < kInverseSteps; ++i) {
    float rad, tx, ty;
    lens_terms(c, x, y, rad, tx, ty);
    ok = ok && rad > 0.0f;
    const float nx = xd - tx;
    const float ny = yd - ty;
    x = nx / rad;
    y = ny / rad;
  }
  return ok && finite(x) && finite(y);
}

__device__ __forceinline__ float pixel_to_ray(int p, float c, float f) {
  const float d = (float)p - c;
  return d / f;
}

__device__ __forceinline__ float ray_to_pixel(float x, float c, float f) {
  const float m = f * x;
  return m + c;
}

// round half to even; false outside the image (and for NaN / inf)
__device__ __forceinline__ bool nearest_index(float us, float vs, int w, int h, int& iu, int& iv) {
  const float ru = __builtin_rintf(us), rv = __builtin_rintf(vs);
  if (!(ru >= 0.0f && ru <= (float)(w - 1) && rv >= 0.0f && rv <= (float)(h - 1))) return false;
  iu = (int)ru;
  iv = (int)rv;
  return true;
}

// the bilinear cell of one axis: i0 = floor(s) in [-1, n - 1] (outside that range every tap is outside: false), f = s - i0
__device__ __forceinline__ bool image_cell(float s, int n, int& i0, float& f) {
  const float fl = __builtin_floorf(s);
  if (!(fl >= -1.0f && fl <= (float)(n - 1))) return false;
  i0 = (int)fl;
  f = s - fl;
  return true;
}

__device__ __forceinline__ float tap(const float* __restrict__ img, int w, int h, int ch, int c, int iu, int iv) {
  if (iu < 0 || iu >= w || iv < 0 || iv >= h) return 0.0f;
  return img[((int64_t)iv * w + iu) * ch + c];
}

// bilinear along u then v, taps outside the image contribute 0
__device__ __forceinline__ float bilinear(const float* __restrict__ img, int w, int h, int ch, int c, int i0, int j0, float fu,
                                          float fv) {
  const float top = lerp(tap(img, w, h, ch, c, i0, j0), tap(img, w, h, ch, c, i0 + 1, j0), fu);
  const float bot = lerp(tap(img, w, h, ch, c, i0, j0 + 1), tap(img, w, h, ch, c, i0 + 1, j0 + 1), fu);
  return lerp(top, bot, fv);
}

// Q = R P + t per row as ((r0 Px + r1 Py) + r2 Pz) + t; T is [4,4] row-major, the same for the whole block (scalar loads)
__device__ __forceinline__ void transform(const float* __restrict__ T, float px, float py, float pz, float& qx, float& qy,
                                          float& qz) {
  qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
  qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
  qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
}

__global__ __launch_bounds__(kRegThreads) void undistort_kernel(const float* __restrict__ src, const Cam cs, const Cam cd,
                                                                const int ch, const int interp, float* __restrict__ dst) {
  int u, v;
  if (!tile_pixel(cd.w, cd.h, u, v)) return;
  const int b = (int)blockIdx.z;
  const float* img = src + (int64_t)b * cs.h * cs.w * ch;
  float* out = dst + (((int64_t)b * cd.h + v) * cd.w + u) * ch;
  const float x = pixel_to_ray(u, cd.cx, cd.fx);
  const float y = pixel_to_ray(v, cd.cy, cd.fy);
  float xd, yd;
  distort(cs, x, y, xd, yd);
  const float us = ray_to_pixel(xd, cs.cx, cs.fx);
  const float vs = ray_to_pixel(yd, cs.cy, cs.fy);
  if (interp == 0) {
    int iu, iv;
    const bool in = nearest_index(us, vs, cs.w, cs.h, iu, iv);
    for (int c = 0; c < ch; ++c) out[c] = in ? img[((int64_t)iv * cs.w + iu) * ch + c] : 0.0f;
  } else {
    int i0, j0;
    float fu, fv;
    const bool in = image_cell(us, cs.w, i0, fu) && image_cell(vs, cs.h, j0, fv);  // (a non-finite coordinate has no cell)
    for (int c = 0; c < ch; ++c) out[c] = in ? bilinear(img, cs.w, cs.h, ch, c, i0, j0, fu, fv) : 0.0f;
  }
}

__global__ __launch_bounds__(256) void fill_kernel(unsigned* __restrict__ zbuf, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) zbuf[i] = kInfBits;
}

__global__ __launch_bounds__(256) void finish_kernel(unsigned* __restrict__ zbuf, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (zbuf[i] == kInfBits) zbuf[i] = 0u;  // +inf (nothing landed) -> 0.0f
}

// the integer pixels of [s - h, s + h] inside [0, n - 1]; false if there is none (or s is not finite)
__device__ __forceinline__ bool footprint(float s, float h, int n, int& lo, int& hi) {
  if (!finite(s)) return false;  // (fmaxf / fminf below would turn a NaN into the whole image)
  const float a = s - h;
  const float b = s + h;
  float l = __builtin_ceilf(a), r = __builtin_floorf(b);
  l = fmaxf(l, 0.0f);
  r = fminf(r, (float)(n - 1));
  if (!(l <= r)) return false;  // (after the two clamps l <= r puts both inside [0, n - 1]; h <= 8 + 1/32: at most 17 pixels)
  lo = (int)l;
  hi = (int)r;
  return true;
}

__global__ __launch_bounds__(kRegThreads) void splat_kernel(const float* __restrict__ depth, const Cam cd,
                                                            const float* __restrict__ T_d2c, const Cam cc, const float half_cap,
                                                            unsigned* __restrict__ zbuf) {
  int u, v;
  if (!tile_pixel(cd.w, cd.h, u, v)) return;
  const int b = (int)blockIdx.z;
  const float z = depth[((int64_t)b * cd.h + v) * cd.w + u];
  if (!(z > 0.0f && finite(z))) return;
  float x, y;
  if (!undistort_point(cd, pixel_to_ray(u, cd.cx, cd.fx), pixel_to_ray(v, cd.cy, cd.fy), x, y)) return;
  const float px = x * z;
  const float py = y * z;
  float qx, qy, qz;
  transform(T_d2c + 16 * (int64_t)b, px, py, z, qx, qy, qz);
  if (!(qz > 0.0f && finite(qz))) return;
  const float xq = qx / qz;
  const float yq = qy / qz;
  const float uc = ray_to_pixel(xq, cc.cx, cc.fx);
  const float vc = ray_to_pixel(yq, cc.cy, cc.fy);
  // the depth pixel's size in colour pixels (the rig's rotation and the lenses ignored), halved, capped, inflated by 1/32
  const float zr = z / qz;
  const float sx = cc.fx / cd.fx;
  const float sy = cc.fy / cd.fy;
  const float hsx = 0.5f * sx;
  const float hsy = 0.5f * sy;
  const float hx = fminf(hsx * zr, half_cap) + 0.03125f;
  const float hy = fminf(hsy * zr, half_cap) + 0.03125f;
  int u0, u1, v0, v1;
  if (!footprint(uc, hx, cc.w, u0, u1) || !footprint(vc, hy, cc.h, v0, v1)) return;
  unsigned* zb = zbuf + (int64_t)b * cc.h * cc.w;
  const unsigned bits = __float_as_uint(qz);  // positive floats order as their bit patterns: min is order-free
  for (int j = v0; j <= v1; ++j)
    for (int i = u0; i <= u1; ++i) atomicMin(zb + (int64_t)j * cc.w + i, bits);
}

struct GatherArgs {
  const float* depth;
  const float* T_d2c;
  const float* color;
  const float* zbuf;  // may be NULL
  float* out_depth;
  float* out_rgb;
  unsigned char* out_valid;
  Cam cd, co, cc, cz;
  float tol;
};

__global__ __launch_bounds__(kRegThreads) void color_to_depth_kernel(const GatherArgs A) {
  int u, v;
  if (!tile_pixel(A.co.w, A.co.h, u, v)) return;
  const int b = (int)blockIdx.z;
  // the depth: nearest sample of the raw image through D_depth, exactly as undistort_kernel with interp = 0
  const float x = pixel_to_ray(u, A.co.cx, A.co.fx);
  const float y = pixel_to_ray(v, A.co.cy, A.co.fy);
  float xd, yd;
  distort(A.cd, x, y, xd, yd);
  int iu, iv;
  float z = 0.0f;
  if (nearest_index(ray_to_pixel(xd, A.cd.cx, A.cd.fx), ray_to_pixel(yd, A.cd.cy, A.cd.fy), A.cd.w, A.cd.h, iu, iv))
    z = A.depth[((int64_t)b * A.cd.h + iv) * A.cd.w + iu];
  bool valid = z > 0.0f && finite(z);
  if (!valid) z = 0.0f;
  // the point on the pinhole ray of (u, v), seen from the colour camera
  const float px = x * z;
  const float py = y * z;
  float qx, qy, qz;
  transform(A.T_d2c + 16 * (int64_t)b, px, py, z, qx, qy, qz);
  valid = valid && qz > 0.0f && finite(qz);
  const float xq = qx / qz;
  const float yq = qy / qz;
  float xc, yc;
  distort(A.cc, xq, yq, xc, yc);
  const float uc = ray_to_pixel(xc, A.cc.cx, A.cc.fx);
  const float vc = ray_to_pixel(yc, A.cc.cy, A.cc.fy);
  int i0 = 0, j0 = 0;
  float fu = 0.0f, fv = 0.0f;
  // VALID needs the whole cell inside the colour image: 0 <= floor <= n - 2 on both axes
  valid = valid && image_cell(uc, A.cc.w, i0, fu) && image_cell(vc, A.cc.h, j0, fv) && i0 >= 0 && i0 <= A.cc.w - 2 && j0 >= 0 &&
          j0 <= A.cc.h - 2;
  if (valid && A.zbuf) {
    int zu, zv;
    if (nearest_index(ray_to_pixel(xq, A.cz.cx, A.cz.fx), ray_to_pixel(yq, A.cz.cy, A.cz.fy), A.cz.w, A.cz.h, zu, zv)) {
      const float zb = A.zbuf[((int64_t)b * A.cz.h + zv) * A.cz.w + zu];
      const float gap = qz - zb;
      if (zb > 0.0f && gap > A.tol) valid = false;  // something nearer was splatted there; zb = 0 (nothing landed) never occludes
    }
  }
  const int64_t pix = ((int64_t)b * A.co.h + v) * A.co.w + u;
  const float* img = A.color + (int64_t)b * A.cc.h * A.cc.w * 3;
  A.out_depth[pix] = z;
  for (int c = 0; c < 3; ++c) A.out_rgb[3 * pix + c] = valid ? bilinear(img, A.cc.w, A.cc.h, 3, c, i0, j0, fu, fv) : 0.0f;
  A.out_valid[pix] = valid ? 1 : 0;
}

bool good_camera(const saf_camera* c) {
  return c && c->width > 0 && c->height > 0 && c->fx > 0.0f && c->fy > 0.0f && isfinite(c->fx) && isfinite(c->fy) &&
         (int64_t)c->width * c->height <= 0x7fffffff;
}

Cam device_camera(const saf_camera* c, bool pinhole) {
  Cam d;
  d.w = c->width;
  d.h = c->height;
  d.fx = c->fx;
  d.fy = c->fy;
  d.cx = c->cx;
  d.cy = c->cy;
  d.k1 = pinhole ? 0.0f : c->dist[0];
  d.k2 = pinhole ? 0.0f : c->dist[1];
  d.p1 = pinhole ? 0.0f : c->dist[2];
  d.p2 = pinhole ? 0.0f : c->dist[3];
  d.k3 = pinhole ? 0.0f : c->dist[4];
  return d;
}

constexpr int kMaxBatch = 65535;  // the grid's third dimension

dim3 tile_grid(const saf_camera* c, int batch) {
  return dim3((unsigned)((c->width + kRegBlock - 1) / kRegBlock), (unsigned)((c->height + kRegBlock - 1) / kRegBlock),
              (unsigned)batch);
}

// (image rows of 16-pixel blocks are the grid's second dimension)
bool good_grid(const saf_camera* c) { return (c->height + kRegBlock - 1) / kRegBlock <= 65535; }

}  // namespace
}  // namespace saf

using namespace saf;

extern "C" {

int saf_undistort_images(const float* src, int32_t batch, int32_t channels, const saf_camera* cam_src, const saf_camera* cam_dst,
                         int32_t interp, float* dst, void* stream) {
  if (!src || !dst || batch <= 0 || batch > kMaxBatch || channels < 1 || channels > 4 || !good_camera(cam_src) ||
      !good_camera(cam_dst) || !good_grid(cam_dst) || (interp != 0 && interp != 1))
    return fail(SAF_E_INVALID, "undistort images: bad arguments (batch %d of at most %d, %d channels of 1 .. 4, interp %d of 0 / 1; "
                "cameras need positive sizes and finite positive fx, fy)", (int)batch, kMaxBatch, (int)channels, (int)interp);
  hipLaunchKernelGGL(undistort_kernel, tile_grid(cam_dst, batch), dim3(kRegThreads), 0, static_cast<hipStream_t>(stream), src,
                     device_camera(cam_src, false), device_camera(cam_dst, true), (int)channels, (int)interp, dst);
  return check_launch("undistort_kernel");
}

size_t saf_depth_to_color_workspace_bytes(int32_t batch, const saf_camera* cam_color) {
  (void)batch;
  (void)cam_color;
  return 0;  // the z-buffer is out_depth itself, reinterpreted
}

int saf_depth_to_color(const float* depth, const saf_camera* cam_depth, const float* T_d2c, int32_t batch,
                       const saf_camera* cam_color, int32_t max_footprint, float* out_depth, void* workspace,
                       size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (!depth || !T_d2c || !out_depth || batch <= 0 || batch > kMaxBatch || !good_camera(cam_depth) || !good_camera(cam_color) ||
      !good_grid(cam_depth) || max_footprint < 1 || max_footprint > 16)
    return fail(SAF_E_INVALID, "depth to color: bad arguments (batch %d of at most %d, max_footprint %d of 1 .. 16; cameras need "
                "positive sizes and finite positive fx, fy)", (int)batch, kMaxBatch, (int)max_footprint);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned* zbuf = reinterpret_cast<unsigned*>(out_depth);
  const int64_t n = (int64_t)batch * cam_color->height * cam_color->width;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_1d(n, 16)), dim3(256), 0, s, zbuf, n);
  hipLaunchKernelGGL(splat_kernel, tile_grid(cam_depth, batch), dim3(kRegThreads), 0, s, depth, device_camera(cam_depth, false),
                     T_d2c, device_camera(cam_color, true), 0.5f * (float)max_footprint, zbuf);
  hipLaunchKernelGGL(finish_kernel, dim3(grid_1d(n, 16)), dim3(256), 0, s, zbuf, n);
  return check_launch("splat_kernel");
}

int saf_color_to_depth(const float* depth, const saf_camera* cam_depth, const saf_camera* cam_depth_out, const float* T_d2c,
                       int32_t batch, const float* color, const saf_camera* cam_color, const float* zbuf,
                       const saf_camera* cam_zbuf, float occlusion_tol, float* out_depth, float* out_rgb, uint8_t* out_valid,
                       void* stream) {
  if (!depth || !T_d2c || !color || !out_depth || !out_rgb || !out_valid || batch <= 0 || batch > kMaxBatch ||
      !good_camera(cam_depth) || !good_camera(cam_depth_out) || !good_camera(cam_color) || !good_grid(cam_depth_out) ||
      (zbuf && !good_camera(cam_zbuf)))
    return fail(SAF_E_INVALID, "color to depth: bad arguments (batch %d of at most %d; cameras need positive sizes and finite "
                "positive fx, fy; a zbuf needs its camera)", (int)batch, kMaxBatch);
  GatherArgs a;
  a.depth = depth;
  a.T_d2c = T_d2c;
  a.color = color;
  a.zbuf = zbuf;
  a.out_depth = out_depth;
  a.out_rgb = out_rgb;
  a.out_valid = out_valid;
  a.cd = device_camera(cam_depth, false);
  a.co = device_camera(cam_depth_out, true);
  a.cc = device_camera(cam_color, false);
  a.cz = device_camera(zbuf ? cam_zbuf : cam_color, true);
  a.tol = occlusion_tol;
  hipLaunchKernelGGL(color_to_depth_kernel, tile_grid(cam_depth_out, batch), dim3(kRegThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("color_to_depth_kernel");
}

}  // extern "C"
