// Colour kernels (gfx950): recolouring of a decoded cloud from the original, and the colour distortion of MPEG pc_error
// 0.13.4 (`--color=1`).  DESIGN.md "Colours" states both rules; tests/_color_ref.py restates them in numpy.
//
// Clouds are voxelised (integer coordinates < res, unique).  The cloud that is SEARCHED becomes the occupancy bit set of
// voxel_grid.h, and every point of the other cloud finds its nearest cells there (nearest_d2, for_each_at_distance).  The
// index of an occupied cell among the cloud's points in key order (key = (x*res + y)*res + z) comes from a rank structure
// over the bit set: the exclusive prefix of the words' popcounts, one 32-bit entry per word, so a cell's index is
// rank[word] + popcount(bits below it) — two loads, no search, no hash table.
//
// Everything that decides an output is integer arithmetic (32-bit atomic adds of colours and counts: order-free), so
// recolouring is defined bit for bit; the colour mse sums float64 terms in a fixed order (per thread, then a tree per
// workgroup, then the workgroups in index order).
#include <algorithm>
#include "common.h"
#include "voxel_grid.h"

namespace pcgc {
namespace {

// ---------------------------------------------------------------------------------------------------------------- bit set + rank
constexpr int kSumBlocks = 1024;
constexpr int64_t kMaxSource = 0xFFFFFFFFll / 255;      // 255 * n_s fits the 32-bit sums of the scatter pass

struct Grid {
  const unsigned* bits;
  const unsigned* rank;      // rank[w] = number of set bits in words 0 .. w-1
  const int64_t* n_set;      // number of set bits (a search over an empty set would never end: it is skipped)
  int res;
};

// index of the occupied cell idx among the set bits in key order
__device__ __forceinline__ int64_t rank_of(const Grid& g, int64_t idx) {
  return rank_of(g.bits, g.rank, idx);
}

// the colours of a cloud in key order, one packed word (r | g << 8 | b << 16) per point
__global__ void colors_to_rank_order_kernel(const int32_t* p, const uint8_t* colors, int64_t n, Grid g, unsigned* packed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  if (!in_grid(g.res, x, y, z)) return;
  packed[rank_of(g, cell_of(g.res, x, y, z))] = (unsigned)colors[i * 3] | ((unsigned)colors[i * 3 + 1] << 8) | ((unsigned)colors[i * 3 + 2] << 16);
}

// ---------------------------------------------------------------------------------------------------------------- search
// squared distance to the nearest occupied cell, kNoCell for an empty set (the shell walk would find nothing, slowly)
__device__ __forceinline__ unsigned nearest_d2(const Grid& g, int x, int y, int z) {
  return *g.n_set == 0 ? kNoCell : nearest_d2(g.bits, g.res, x, y, z);
}

// calls f(j) with the key-order index j of every occupied cell at squared distance `best` from (x, y, z): ties are kept
template <typename F>
__device__ __forceinline__ void for_each_nearest(const Grid& g, int x, int y, int z, unsigned best, F f) {
  if (best == kNoCell) return;
  for_each_at_distance(g.bits, g.res, x, y, z, best, [&](int dx, int dy, int qz) { f(rank_of(g, cell_of(g.res, x + dx, y + dy, qz))); });
}

// mean rounded half up, in integers
__device__ __forceinline__ int rounded_mean(unsigned sum, unsigned n) { return (int)((2ull * sum + n) / (2ull * n)); }

// ---------------------------------------------------------------------------------------------------------------- recolouring
// S -> T: every source point adds its colour and a one to each of its nearest target points.  acc[j] = (sum r, sum g,
// sum b, |B(t_j)|) as four adjacent uint32, so the four adds of a pair touch one 16-byte slot.  A sum is at most 255 n_s:
// pcgc_recolor refuses more source points than 2^32 / 255.
__global__ void __launch_bounds__(256) recolor_scatter_kernel(const int32_t* ps, const uint8_t* cs, int64_t ns, Grid t, unsigned* acc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ns; i += (int64_t)gridDim.x * 256) {
    const int x = ps[i * 3], y = ps[i * 3 + 1], z = ps[i * 3 + 2];
    const unsigned r = cs[i * 3], gch = cs[i * 3 + 1], b = cs[i * 3 + 2];
    for_each_nearest(t, x, y, z, nearest_d2(t, x, y, z), [&](int64_t j) {
      atomicAdd(&acc[j * 4], r);
      atomicAdd(&acc[j * 4 + 1], gch);
      atomicAdd(&acc[j * 4 + 2], b);
      atomicAdd(&acc[j * 4 + 3], 1u);
    });
  }
}

// one thread per target point: the rounded mean of what the scatter left, or of the target's own nearest source points
__global__ void __launch_bounds__(256) recolor_final_kernel(const int64_t* tkeys, int64_t nt, const uint4* acc, Grid s,
                                                            const unsigned* scolors, uint8_t* out, int32_t* counts) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nt) return;
  const uint4 a = acc[j];
  unsigned sr = a.x, sg = a.y, sb = a.z, n = a.w;
  if (counts) counts[j] = (int32_t)n;
  if (n == 0) {
    const int64_t key = tkeys[j], rr = (int64_t)s.res * s.res;
    const int x = (int)(key / rr), y = (int)((key / s.res) % s.res), z = (int)(key % s.res);
    for_each_nearest(s, x, y, z, nearest_d2(s, x, y, z), [&](int64_t i) {
      const unsigned c = scolors[i];
      sr += c & 255u; sg += (c >> 8) & 255u; sb += (c >> 16) & 255u;
      ++n;
    });
  }
  out[j * 3] = n ? (uint8_t)rounded_mean(sr, n) : 0;
  out[j * 3 + 1] = n ? (uint8_t)rounded_mean(sg, n) : 0;
  out[j * 3 + 2] = n ? (uint8_t)rounded_mean(sb, n) : 0;
}

// ---------------------------------------------------------------------------------------------------------------- colour mse
// BT.709 of rgb / 255, written term by term in the order of the numpy statement (the file is built with -ffp-contract=off)
__device__ __forceinline__ void yuv_bt709(int r8, int g8, int b8, double yuv[3]) {
  const double r = (double)r8 / 255.0, g = (double)g8 / 255.0, b = (double)b8 / 255.0;
  yuv[0] = 0.2126 * r + 0.7152 * g + 0.0722 * b;
  yuv[1] = -0.1146 * r - 0.3854 * g + 0.5 * b + 0.5;
  yuv[2] = 0.5 * r - 0.4542 * g - 0.0458 * b + 0.5;
}

__global__ void __launch_bounds__(256) color_mse_partial_kernel(const int32_t* pa, const uint8_t* ca, int64_t na, Grid b,
                                                                const unsigned* bcolors, double* partial) {
  __shared__ double sh[3][256];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na; i += (int64_t)gridDim.x * 256) {
    const int x = pa[i * 3], y = pa[i * 3 + 1], z = pa[i * 3 + 2];
    unsigned sr = 0, sg = 0, sb = 0, n = 0;
    for_each_nearest(b, x, y, z, nearest_d2(b, x, y, z), [&](int64_t j) {
      const unsigned c = bcolors[j];
      sr += c & 255u; sg += (c >> 8) & 255u; sb += (c >> 16) & 255u;
      ++n;
    });
    if (n == 0) continue;
    double ya[3], yb[3];
    yuv_bt709(ca[i * 3], ca[i * 3 + 1], ca[i * 3 + 2], ya);
    yuv_bt709(rounded_mean(sr, n), rounded_mean(sg, n), rounded_mean(sb, n), yb);
    for (int c = 0; c < 3; ++c) acc[c] += (ya[c] - yb[c]) * (ya[c] - yb[c]);
  }
  for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] = acc[c];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void color_mse_final_kernel(const double* partial, int nb, int64_t na, double* out3) {
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += partial[i * 3 + threadIdx.x];
    out3[threadIdx.x] = s / (double)na;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool sizes_ok(int res, int64_t a, int64_t b) {
  return res > 0 && res <= 4096 && a > 0 && b > 0 && a <= 0x7FFFFFFF && b <= 0x7FFFFFFF;
}

// the rank structure of one cloud, then pcgc_recolor's accumulators per target [n_t, 4] and source colours by rank [n_s]
struct RecolorBuffers { RankBuffers r; unsigned *acc, *scolors; size_t bytes; };

RecolorBuffers recolor_layout(int res, int64_t n_s, int64_t n_t, void* workspace) {
  RecolorBuffers b;
  b.r = rank_layout(res, workspace);
  Carver& c = b.r.rest;
  b.acc = c.take<unsigned>((size_t)n_t * 4);
  b.scolors = c.take<unsigned>((size_t)n_s);
  b.bytes = c.bytes();
  return b;
}

// ... then pcgc_color_mse's colours of B by rank [n_b] and the partial sums [3, kSumBlocks]
struct ColorMseBuffers { RankBuffers r; unsigned* bcolors; double* partial; size_t bytes; };

ColorMseBuffers color_mse_layout(int res, int64_t n_b, void* workspace) {
  ColorMseBuffers b;
  b.r = rank_layout(res, workspace);
  Carver& c = b.r.rest;
  b.bcolors = c.take<unsigned>((size_t)n_b);
  b.partial = c.take<double>(3 * kSumBlocks);
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_recolor_workspace_bytes(int res, int64_t n_s, int64_t n_t) {
  return sizes_ok(res, n_s, n_t) && n_s <= kMaxSource ? recolor_layout(res, n_s, n_t, nullptr).bytes : 0;
}

int pcgc_recolor(const int32_t* source_points, const uint8_t* source_colors, int64_t n_s, const int64_t* target_keys, int64_t n_t,
                 int res, uint8_t* target_colors, int32_t* backward_counts, void* workspace, size_t workspace_bytes,
                 pcgc_stream_t stream) {
  PCGC_REQUIRE(source_points && source_colors && target_keys && target_colors && workspace && sizes_ok(res, n_s, n_t),
               "pcgc_recolor: bad arguments");
  PCGC_REQUIRE(n_s <= kMaxSource, "pcgc_recolor: %lld source points, the 32-bit colour sums hold %lld", (long long)n_s, (long long)kMaxSource);
  const RecolorBuffers b = recolor_layout(res, n_s, n_t, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_recolor: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const RankBuffers& r = b.r;
  const Grid g{r.bits, r.rank, r.n_set, res};
  // the target's rank structure, then S -> T
  int rc = build_rank(r, res, nullptr, target_keys, n_t, s);
  if (rc) return rc;
  PCGC_CHECK_HIP(hipMemsetAsync(b.acc, 0, (size_t)n_t * 4 * sizeof(unsigned), s));
  const int blocks = (int)std::min<int64_t>((n_s + 255) / 256, 4096);
  hipLaunchKernelGGL(recolor_scatter_kernel, dim3(blocks), dim3(256), 0, s, source_points, source_colors, n_s, g, b.acc);
  // the same memory becomes the source's rank structure for the targets that nothing reached
  rc = build_rank(r, res, source_points, nullptr, n_s, s);
  if (rc) return rc;
  hipLaunchKernelGGL(colors_to_rank_order_kernel, dim3((unsigned)((n_s + 255) / 256)), dim3(256), 0, s, source_points, source_colors,
                     n_s, g, b.scolors);
  hipLaunchKernelGGL(recolor_final_kernel, dim3((unsigned)((n_t + 255) / 256)), dim3(256), 0, s, target_keys, n_t,
                     reinterpret_cast<const uint4*>(b.acc), g, b.scolors, target_colors, backward_counts);
  return launch_ok("recolor kernels");
}

size_t pcgc_color_mse_workspace_bytes(int res, int64_t n_b) {
  return sizes_ok(res, 1, n_b) ? color_mse_layout(res, n_b, nullptr).bytes : 0;
}

int pcgc_color_mse(const int32_t* points_a, const uint8_t* colors_a, int64_t n_a, const int32_t* points_b, const uint8_t* colors_b,
                   int64_t n_b, int res, double* out3, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points_a && colors_a && points_b && colors_b && out3 && workspace && sizes_ok(res, n_a, n_b),
               "pcgc_color_mse: bad arguments");
  const ColorMseBuffers b = color_mse_layout(res, n_b, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_color_mse: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const RankBuffers& r = b.r;
  const Grid g{r.bits, r.rank, r.n_set, res};
  int rc = build_rank(r, res, points_b, nullptr, n_b, s);
  if (rc) return rc;
  hipLaunchKernelGGL(colors_to_rank_order_kernel, dim3((unsigned)((n_b + 255) / 256)), dim3(256), 0, s, points_b, colors_b, n_b, g,
                     b.bcolors);
  const int blocks = (int)std::min<int64_t>((n_a + 255) / 256, kSumBlocks);
  hipLaunchKernelGGL(color_mse_partial_kernel, dim3(blocks), dim3(256), 0, s, points_a, colors_a, n_a, g, b.bcolors, b.partial);
  hipLaunchKernelGGL(color_mse_final_kernel, dim3(1), dim3(64), 0, s, b.partial, blocks, n_a, out3);
  return launch_ok("colour mse kernels");
}

}  // extern "C"
