// Point clouds to images (gfx950): orthographic projection, hidden-point removal by a 64-bit z-buffer, eye-dome lighting,
// and a colour map for per-point error figures.  DESIGN.md "Rendering" states the rule; tests/_render_ref.py restates it
// in numpy.  Everything after one rounding of the coordinates is integer arithmetic, so the image is defined bit for bit.
//
//   splat    one thread per point (grid-stride): q = rintf(p * 16), t = (R q + 8192) >> 14, pixel and depth from the window;
//            key = depth << 32 | index goes into every pixel of the point's square with one 64-bit atomic min.  The
//            minimum of distinct keys does not depend on arrival order; a pixel whose stored key is already smaller is
//            left alone without an atomic (a stale read can only be too large, which costs an atomic, never a result).
//   resolve  one thread per pixel: the winner's colour, shaded by the depth steps to the eight neighbours.
//   colormap one thread per value (grid-stride): a 256-entry table looked up at floor(value * scale).
//
// Every pixel index is clipped to the image before it is used and every point index is compared with n before it reads
// a colour, so no input — a NaN, a coordinate outside the stated range, a z-buffer some other call filled — indexes
// outside a buffer.
#include <algorithm>
#include <cmath>
#include "common.h"

namespace pcgc {
namespace {

constexpr int kRenderMaxSide = 8192;
constexpr int kRenderMaxPointSize = 15;
constexpr int64_t kRenderMaxPoints = 0xFFFFFFFFll - 1;       // n < 2^32 - 1: an index fits the key's low word
constexpr int64_t kRenderMaxOffset = (int64_t)1 << 31;       // |u0|, |v1|, |w1| stay below it
constexpr int kRenderMaxScale = 1 << 30;                     // (t - u0) * S then stays below 2^63
constexpr int kRenderMaxShift = 1 << 20;                     // |ox|, |oy|
constexpr int kRenderMaxShade = 1 << 20;
constexpr float kRenderMaxQ = 524288.0f;                     // 2^19 = 16 * 2^15: |q| of every coordinate inside the contract
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kSplatBlocks = 2048;

struct View {
  int32_t r[9];              // Q14, rows right, up, toward the viewer
  int64_t u0, v1, w1;
  int32_t s, ox, oy;
  int width, height, half;   // half = point_size / 2
};

__global__ void __launch_bounds__(256) render_splat_kernel(const float* p, int64_t n, View v, unsigned long long* zbuf) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t q[3];
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
      const float f = rintf(p[i * 3 + a] * 16.0f);           // round half to even; 1/16-voxel units
      ok = ok && fabsf(f) <= kRenderMaxQ;                    // false for a NaN
      q[a] = ok ? (int64_t)f : 0;
    }
    if (!ok) continue;
    int64_t t[3];
    for (int r = 0; r < 3; ++r) t[r] = ((int64_t)v.r[r * 3] * q[0] + (int64_t)v.r[r * 3 + 1] * q[1] + (int64_t)v.r[r * 3 + 2] * q[2] + 8192) >> 14;
    const int64_t px = (((t[0] - v.u0) * v.s) >> 16) + v.ox;
    const int64_t py = (((v.v1 - t[1]) * v.s) >> 16) + v.oy;
    const int64_t d = v.w1 - t[2];
    if (d < 0 || d >= ((int64_t)1 << 31)) continue;
    const int64_t x0 = max(px - v.half, (int64_t)0), x1 = min(px + v.half, (int64_t)v.width - 1);
    const int64_t y0 = max(py - v.half, (int64_t)0), y1 = min(py + v.half, (int64_t)v.height - 1);
    const unsigned long long key = ((unsigned long long)d << 32) | (unsigned long long)(uint32_t)i;
    for (int64_t y = y0; y <= y1; ++y)
      for (int64_t x = x0; x <= x1; ++x) {
        unsigned long long* z = zbuf + y * v.width + x;
        if (*z > key) atomicMin(z, key);
      }
  }
}

struct Shade {
  int width, height, k;
  uint32_t background, foreground;       // 0xRRGGBB
};

__global__ void __launch_bounds__(256) render_resolve_kernel(const unsigned long long* zbuf, Shade s, const uint8_t* colors, int64_t n,
                                                             uint8_t* rgb, int32_t* index, int32_t* depth) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (int64_t)s.width * s.height) return;
  const int x = (int)(pix % s.width), y = (int)(pix / s.width);
  const unsigned long long key = zbuf[pix];
  if (key == kEmpty) {
    for (int c = 0; c < 3; ++c) rgb[pix * 3 + c] = (uint8_t)(s.background >> (16 - 8 * c));
    if (index) index[pix] = -1;
    if (depth) depth[pix] = -1;
    return;
  }
  const int64_t d = (int64_t)(key >> 32), i = (int64_t)(key & 0xFFFFFFFFull);
  int64_t shade = 255;
  if (s.k > 0) {
    int64_t obs = 0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int nx = x + dx, ny = y + dy;
        if ((dx == 0 && dy == 0) || (unsigned)nx >= (unsigned)s.width || (unsigned)ny >= (unsigned)s.height) continue;
        const unsigned long long nk = zbuf[(int64_t)ny * s.width + nx];
        if (nk != kEmpty) obs += max(d - (int64_t)(nk >> 32), (int64_t)0);
      }
    shade = (255 * (int64_t)s.k) / ((int64_t)s.k + obs);
  }
  const bool own = colors != nullptr && i < n;
  for (int c = 0; c < 3; ++c) {
    const int64_t base = own ? colors[i * 3 + c] : (uint8_t)(s.foreground >> (16 - 8 * c));
    rgb[pix * 3 + c] = (uint8_t)((base * shade + 127) / 255);
  }
  if (index) index[pix] = (int32_t)(uint32_t)i;
  if (depth) depth[pix] = (int32_t)d;
}

__global__ void __launch_bounds__(256) colormap_kernel(const float* values, int64_t n, float scale, const uint8_t* lut, uint8_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float f = floorf(values[i] * scale);
    const int bin = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);      // a NaN or a negative value takes bin 0
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = lut[bin * 3 + c];
  }
}

bool image_ok(int width, int height) { return width >= 1 && width <= kRenderMaxSide && height >= 1 && height <= kRenderMaxSide; }

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_render_workspace_bytes(int width, int height) {
  if (!image_ok(width, height)) return 0;
  return (size_t)width * height * sizeof(unsigned long long);
}

int pcgc_render_splat(const float* points, int64_t n, const int32_t* rotation, int64_t u0, int64_t v1, int64_t w1, int32_t scale,
                      int32_t ox, int32_t oy, int width, int height, int point_size, void* workspace, size_t workspace_bytes,
                      pcgc_stream_t stream) {
  PCGC_REQUIRE(rotation && workspace && (points || n == 0), "pcgc_render_splat: null pointer");
  PCGC_REQUIRE(image_ok(width, height), "pcgc_render_splat: width and height must lie within 1..%d (got %d x %d)", kRenderMaxSide, width,
               height);
  PCGC_REQUIRE(point_size >= 1 && point_size <= kRenderMaxPointSize && (point_size & 1),
               "pcgc_render_splat: point_size must be odd and within 1..%d (got %d)", kRenderMaxPointSize, point_size);
  PCGC_REQUIRE(n >= 0 && n < kRenderMaxPoints, "pcgc_render_splat: n must lie within [0, 2^32 - 1) (got %lld)", (long long)n);
  PCGC_REQUIRE(workspace_bytes >= pcgc_render_workspace_bytes(width, height) && (uintptr_t)workspace % sizeof(unsigned long long) == 0,
               "pcgc_render_splat: workspace too small or not 8-byte aligned");
  View v;
  for (int k = 0; k < 9; ++k) {
    PCGC_REQUIRE(rotation[k] >= -16384 && rotation[k] <= 16384, "pcgc_render_splat: rotation entries are Q14, within [-16384, 16384]");
    v.r[k] = rotation[k];
  }
  PCGC_REQUIRE(u0 > -kRenderMaxOffset && u0 < kRenderMaxOffset && v1 > -kRenderMaxOffset && v1 < kRenderMaxOffset &&
               w1 > -kRenderMaxOffset && w1 < kRenderMaxOffset, "pcgc_render_splat: window offsets must lie within (-2^31, 2^31)");
  PCGC_REQUIRE(scale >= 1 && scale <= kRenderMaxScale && ox >= -kRenderMaxShift && ox <= kRenderMaxShift && oy >= -kRenderMaxShift &&
               oy <= kRenderMaxShift, "pcgc_render_splat: window scale must lie within 1..2^30 and the pixel offsets within +-2^20");
  v.u0 = u0; v.v1 = v1; v.w1 = w1;
  v.s = scale; v.ox = ox; v.oy = oy;
  v.width = width; v.height = height; v.half = point_size / 2;
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemsetAsync(workspace, 0xFF, pcgc_render_workspace_bytes(width, height), s));
  if (n == 0) return 0;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, kSplatBlocks);
  hipLaunchKernelGGL(render_splat_kernel, dim3(blocks), dim3(256), 0, s, points, n, v, reinterpret_cast<unsigned long long*>(workspace));
  return launch_ok("render splat kernel");
}

int pcgc_render_resolve(const void* workspace, size_t workspace_bytes, int width, int height, const uint8_t* colors, int64_t n,
                        uint32_t background, uint32_t foreground, int shade, uint8_t* rgb, int32_t* index, int32_t* depth,
                        pcgc_stream_t stream) {
  PCGC_REQUIRE(workspace && rgb, "pcgc_render_resolve: null pointer");
  PCGC_REQUIRE(image_ok(width, height), "pcgc_render_resolve: width and height must lie within 1..%d (got %d x %d)", kRenderMaxSide,
               width, height);
  PCGC_REQUIRE(n >= 0 && n < kRenderMaxPoints, "pcgc_render_resolve: n must lie within [0, 2^32 - 1) (got %lld)", (long long)n);
  PCGC_REQUIRE(workspace_bytes >= pcgc_render_workspace_bytes(width, height) && (uintptr_t)workspace % sizeof(unsigned long long) == 0,
               "pcgc_render_resolve: workspace too small or not 8-byte aligned");
  PCGC_REQUIRE(shade >= 0 && shade <= kRenderMaxShade && background <= 0xFFFFFFu && foreground <= 0xFFFFFFu,
               "pcgc_render_resolve: shade must lie within 0..2^20 and the colours within 0xRRGGBB");
  PCGC_REQUIRE((uintptr_t)index % sizeof(int32_t) == 0 && (uintptr_t)depth % sizeof(int32_t) == 0,
               "pcgc_render_resolve: index and depth must be 4-byte aligned");
  const Shade sh{width, height, shade, background, foreground};
  const unsigned blocks = (unsigned)(((int64_t)width * height + 255) / 256);
  hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(workspace), sh, colors, n, rgb, index, depth);
  return launch_ok("render resolve kernel");
}

int pcgc_colormap(const float* values, int64_t n, float scale, const uint8_t* lut, uint8_t* out, pcgc_stream_t stream) {
  PCGC_REQUIRE(n >= 0, "pcgc_colormap: n must not be negative (got %lld)", (long long)n);
  if (n == 0) return 0;
  PCGC_REQUIRE(values && lut && out, "pcgc_colormap: null pointer");
  PCGC_REQUIRE(scale >= 0.0f && std::isfinite(scale), "pcgc_colormap: scale must be finite and not negative");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(colormap_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, values, n, scale, lut, out);
  return launch_ok("colormap kernel");
}

}  // extern "C"
