// Global alignment of two scans (gfx950): the four device stages of pcgcv1_amd/register.py's global_align.  include/pcgc.h
// (pcgc_feature_*, pcgc_ransac_score) and DESIGN.md §7i state the rule; tests/_global_ref.py restates it in numpy by brute force.
//
//   1. pairs:   per keypoint i, three 11-bin histograms over its neighbours j within r of |n_i . u|, |n_j . u| and |n_i . n_j|
//               (u the unit vector between them): sign-invariant, because the normals the project estimates are unoriented.
//   2. combine: a keypoint's histogram and its neighbours' into one row of 33 bytes, all in integers.
//   3. match:   per source row the target row with the smallest sum of squared byte differences, brute force.
//   4. score:   per trial pose the number of correspondences it brings within a distance.
// Every output is an integer that does not depend on the order the work is done in, so the device and numpy agree bit for bit.
// The float64 arithmetic in front of the binning is one operation per step in the order written (-ffp-contract=off).
//
// Stages 1 and 2 walk the cells of offgrid_cells.h (window_of, for_each_run): one wave per keypoint, the cells of the window of
// r around its cell in wave-uniform loops, the lanes over the points of a cell.  The histogram of stage 1 lives in LDS (33 counters per wave,
// integer atomicAdd): counters indexed by a run-time bin would otherwise spill to scratch.  Stage 2 needs no atomics: the
// lanes agree by ballot on the neighbours of a chunk, then lane b < 33 adds bin b of each.
// Input that breaks the contract (keypoints not sorted by cell or outside the grid, a NaN coordinate) is met with no index
// out of bounds: it raises the flag in the workspace, and the outputs say so (k = -1, valid = 255).
#include <algorithm>
#include <cmath>
#include "common.h"
#include "offgrid_cells.h"

namespace pcgc {
namespace {

constexpr int kBins = 11, kCounters = 3 * kBins, kRowBytes = 36, kRowWords = kRowBytes / 4;
constexpr int kFeatureMaxWindow = 4;                // cells each way: floor(r / h) + 1 <= 4, at most 9^3 cells per keypoint
constexpr int64_t kFeatureMaxPoints = 1 << 24;      // k < 2^24, so T = k^2 + sum of k < 2^49 and G * 255 fits 64 bits
constexpr int kFeatureBlocks = 4096;
constexpr int kMatchTile = 256, kMatchTileWords = 12;                   // a staged row is padded to 48 bytes: 16-byte reads
constexpr unsigned kNoRow = 0xFFFFFFFFu;

__device__ __forceinline__ bool usable_normal(const float* n) {
  const bool finite = fabsf(n[0]) < INFINITY && fabsf(n[1]) < INFINITY && fabsf(n[2]) < INFINITY;
  return finite && (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f);
}

// min(10, (int)floor(f * 11.0)) for f >= 0; a NaN lands in bin 10
__device__ __forceinline__ int bin_of(double f) {
  const double x = f * 11.0;
  return x < 10.0 ? (int)floor(x) : 10;
}

// is j a neighbour of i (at p): j != i, 0 < d2 <= r2, a usable normal; d = p - q_j
__device__ __forceinline__ bool is_neighbour(const Target& t, const float* normals, int64_t i, int32_t j, double px, double py, double pz,
                                             double r2, double d[3], double* d2) {
  const float* q = t.q + (int64_t)j * 3;
  d[0] = px - (double)q[0];
  d[1] = py - (double)q[1];
  d[2] = pz - (double)q[2];
  *d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  return j != i && *d2 > 0.0 && *d2 <= r2 && usable_normal(normals + (int64_t)j * 3);
}

// ---------------------------------------------------------------------------------------------------------------- 1: pairs
// One wave per keypoint, four keypoints per workgroup pass; every wave takes every pass, so the barriers are uniform.
__global__ void __launch_bounds__(256) feature_pairs_kernel(Target t, const float* normals, int64_t n, int w, double r2, uint32_t* S,
                                                            int32_t* k, int* bad) {
  __shared__ unsigned hist[4][kCounters];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t i = base + wave;
    const bool active = i < n;
    if (lane < kCounters) hist[wave][lane] = 0u;
    __syncthreads();
    int count = 0;
    int cell[3];
    bool walk = false;
    if (active) {
      walk = cell_of_point(t.c, t.q + i * 3, cell);
      if (!walk && lane == 0) atomicOr(bad, 1);
      walk = walk && usable_normal(normals + i * 3);
    }
    if (walk) {
      const double px = t.q[i * 3], py = t.q[i * 3 + 1], pz = t.q[i * 3 + 2];
      const double nx = normals[i * 3], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
      for_each_run(t, window_of(cell, w, t.c.res), [&](int32_t first, int32_t end) {
        for (int32_t j = first + lane; j < end; j += 64) {
          double d[3], d2;
          if (!is_neighbour(t, normals, i, j, px, py, pz, r2, d, &d2)) continue;
          const double len = sqrt(d2);
          const double ux = d[0] / len, uy = d[1] / len, uz = d[2] / len;
          const double mx = normals[(int64_t)j * 3], my = normals[(int64_t)j * 3 + 1], mz = normals[(int64_t)j * 3 + 2];
          const double f1 = fabs((nx * ux + ny * uy) + nz * uz);
          const double f2 = fabs((mx * ux + my * uy) + mz * uz);
          const double f3 = fabs((nx * mx + ny * my) + nz * mz);
          atomicAdd(&hist[wave][bin_of(f1)], 1u);
          atomicAdd(&hist[wave][kBins + bin_of(f2)], 1u);
          atomicAdd(&hist[wave][2 * kBins + bin_of(f3)], 1u);
          ++count;
        }
      });
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_down(count, o, 64);
    __syncthreads();
    if (active) {
      if (lane < kCounters) S[i * kCounters + lane] = hist[wave][lane];
      if (lane == 0) k[i] = count;
    }
    __syncthreads();
  }
}

// what a raised flag does to the output of stage 1: k = -1 (stage 2: valid = 255, flag_marks_kernel of offgrid_cells.h)
__global__ void __launch_bounds__(256) feature_flag_kernel(const int* bad, int64_t n, int32_t* k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !*bad) return;
  k[i] = -1;
}

// ---------------------------------------------------------------------------------------------------------------- 2: combine
__global__ void __launch_bounds__(256) feature_combine_kernel(Target t, const float* normals, int64_t n, int w, double r2, const uint32_t* S,
                                                              const int32_t* k, uint8_t* feat, uint8_t* valid, int* bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n; i += (int64_t)gridDim.x * 4) {       // no barrier: the waves are on their own
    unsigned long long acc = 0;                            // lane b < 33: sum of S_j[b]; lane 33: sum of k_j
    int cell[3];
    bool walk = cell_of_point(t.c, t.q + i * 3, cell);
    if (!walk && lane == 0) atomicOr(bad, 1);
    walk = walk && usable_normal(normals + i * 3);
    if (walk) {
      const double px = t.q[i * 3], py = t.q[i * 3 + 1], pz = t.q[i * 3 + 2];
      for_each_run(t, window_of(cell, w, t.c.res), [&](int32_t first, int32_t end) {
        for (; first < end; first += 64) {
          const int32_t j = first + lane;
          double d[3], d2;
          const bool member = j < end && is_neighbour(t, normals, i, j, px, py, pz, r2, d, &d2);
          unsigned long long mask = __ballot(member);
          while (mask) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int64_t jj = (int64_t)first + b;
            if (lane < kCounters) acc += S[jj * kCounters + lane];
            else if (lane == kCounters) acc += (unsigned)k[jj];
          }
        }
      });
    }
    const unsigned long long ki = (unsigned)k[i];
    const unsigned long long T = ki * ki + __shfl(acc, kCounters, 64);
    unsigned long long byte = 0;
    if (lane < kCounters && T > 0) {
      const unsigned long long G = ki * S[i * kCounters + lane] + acc;
      byte = min((G * 255ull + T / 2ull) / T, 255ull);
    }
    if (lane < kRowBytes) feat[i * kRowBytes + lane] = (uint8_t)byte;
    if (lane == 0) valid[i] = T > 0 ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- 3: match
// sum of the products of the four bytes of a and b.  v_dot4_u32_u8 where the compiler offers it for the target.
__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c) {
#if __has_builtin(__builtin_amdgcn_udot4)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

// the nine words of a row, the three bytes behind the 33 bins masked out; *norm = the sum of its squared bytes
__device__ __forceinline__ void load_row(const uint8_t* rows, int64_t i, unsigned a[kRowWords], unsigned* norm) {
  const unsigned* src = reinterpret_cast<const unsigned*>(rows + i * kRowBytes);
  unsigned s = 0;
#pragma unroll
  for (int c = 0; c < kRowWords; ++c) {
    a[c] = src[c];
    if (c == kRowWords - 1) a[c] &= 0xFFu;
    s = dot4(a[c], a[c], s);
  }
  *norm = s;
}

// One thread per source row, the rows of blockIdx.y's share of the target staged in LDS a tile at a time: every lane reads the
// same staged row, a broadcast.  |a - b|^2 = |a|^2 + |b|^2 - 2 a.b, exact in 32 bits (at most 33 * 255^2).  best[i] = the least
// (distance << 32 | target row) over the shares: the least distance, and among equals the lowest row.
__global__ void __launch_bounds__(256) feature_match_kernel(const uint8_t* fs, const uint8_t* vs, int64_t n, const uint8_t* ft,
                                                            const uint8_t* vt, int64_t m, int64_t tiles_per_share,
                                                            unsigned long long* best) {
  __shared__ __align__(16) unsigned tile[kMatchTile][kMatchTileWords];
  __shared__ unsigned norms[kMatchTile];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n && vs[i] != 0;
  unsigned a[kRowWords], na = 0;
#pragma unroll
  for (int c = 0; c < kRowWords; ++c) a[c] = 0u;
  if (live) load_row(fs, i, a, &na);
  unsigned long long least = ~0ull;
  const int64_t n_tiles = (m + kMatchTile - 1) / kMatchTile;
  const int64_t t0 = (int64_t)blockIdx.y * tiles_per_share, t1 = std::min<int64_t>(t0 + tiles_per_share, n_tiles);
  for (int64_t tl = t0; tl < t1; ++tl) {
    const int64_t row0 = tl * kMatchTile, j = row0 + threadIdx.x;
    __syncthreads();
    unsigned b[kRowWords], nb = kNoRow;
#pragma unroll
    for (int c = 0; c < kRowWords; ++c) b[c] = 0u;
    if (j < m && vt[j] != 0) load_row(ft, j, b, &nb);
#pragma unroll
    for (int c = 0; c < kRowWords; ++c) tile[threadIdx.x][c] = b[c];
    norms[threadIdx.x] = nb;
    __syncthreads();
    const int rows = (int)std::min<int64_t>(kMatchTile, m - row0);
    for (int r = 0; r < rows; ++r) {
      const unsigned nr = norms[r];
      if (nr == kNoRow) continue;                            // the same row in every lane: a uniform branch
      unsigned dot = 0;
#pragma unroll
      for (int c = 0; c < kRowWords; ++c) dot = dot4(a[c], tile[r][c], dot);
      const unsigned long long key = ((unsigned long long)(na + nr - 2u * dot) << 32) | (unsigned long long)(row0 + r);
      least = key < least ? key : least;
    }
  }
  if (live && least != ~0ull) atomicMin(&best[i], least);
}

__global__ void __launch_bounds__(256) feature_match_final_kernel(const unsigned long long* best, int64_t n, int32_t* j, uint32_t* dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = best[i];                   // untouched: all ones, which reads as row -1 at distance 0xFFFFFFFF
  j[i] = (int32_t)(unsigned)(key & 0xFFFFFFFFull);
  dist[i] = (uint32_t)(key >> 32);
}

// ---------------------------------------------------------------------------------------------------------------- 4: score
// One workgroup per pose in turn, its threads over the correspondences; the count is reduced in integers.
__global__ void __launch_bounds__(256) ransac_score_kernel(const double* poses, int64_t n_poses, const float* P, const float* Q, int64_t C,
                                                           double gate2, int32_t* counts) {
  __shared__ int part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t k = blockIdx.x; k < n_poses; k += gridDim.x) {
    double R[9], t[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = poses[k * 12 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = poses[k * 12 + 9 + c];
    int count = 0;
    for (int64_t c = threadIdx.x; c < C; c += 256) {
      const double x = P[c * 3], y = P[c * 3 + 1], z = P[c * 3 + 2];
      float pf[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) pf[r] = (float)(((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t[r]);
      count += dist2(Q + c * 3, (double)pf[0], (double)pf[1], (double)pf[2]) <= gate2 ? 1 : 0;          // false for a NaN
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_down(count, o, 64);
    if (lane == 0) part[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) counts[k] = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool feature_sizes_ok(int res, int64_t n) { return res >= 1 && res <= kOffgridMaxRes && n > 0 && n <= kFeatureMaxPoints; }

// the window of r in cells of edge h: a point within r of p lies at most floor(r / h) + 1 cells from p's cell
bool window_ok(double radius, double h, int* w) {
  if (!(std::isfinite(radius) && radius > 0.0) || !edge_ok(h)) return false;
  const double cells = std::floor(radius / h) + 1.0;
  if (!(cells <= (double)kFeatureMaxWindow)) return false;
  *w = (int)cells;
  return true;
}

int feature_blocks(int64_t n) { return (int)std::min<int64_t>((n + 3) / 4, kFeatureBlocks); }

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_feature_workspace_bytes(int res, int64_t n) { return feature_sizes_ok(res, n) ? cell_buffer_layout(res, n, nullptr).bytes : 0; }

int pcgc_feature_pairs(const float* kp, const float* normals, int64_t n, double h, int ox, int oy, int oz, int res, double radius,
                       uint32_t* S, int32_t* k, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  int w = 0;
  PCGC_REQUIRE(kp && normals && S && k && workspace && feature_sizes_ok(res, n) && grid_ok(h, ox, oy, oz, res, n, n),
               "pcgc_feature_pairs: bad arguments");
  PCGC_REQUIRE(window_ok(radius, h, &w), "pcgc_feature_pairs: radius %g must be positive and below %d cells of edge %g", radius,
               kFeatureMaxWindow, h);
  const CellBuffers b = cell_buffer_layout(res, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_feature_pairs: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_cells(b.r, b.keys, b.start, b.bad, Cells{h, ox, oy, oz, res}, kp, n, s, &t);
  if (rc) return rc;
  hipLaunchKernelGGL(feature_pairs_kernel, dim3(feature_blocks(n)), dim3(256), 0, s, t, normals, n, w, radius * radius, S, k, b.bad);
  hipLaunchKernelGGL(feature_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b.bad, n, k);
  return launch_ok("feature pair kernels");
}

int pcgc_feature_combine(const float* kp, const float* normals, int64_t n, double h, int ox, int oy, int oz, int res, double radius,
                         const uint32_t* S, const int32_t* k, uint8_t* feat, uint8_t* valid, void* workspace, size_t workspace_bytes,
                         pcgc_stream_t stream) {
  int w = 0;
  PCGC_REQUIRE(kp && normals && S && k && feat && valid && workspace && feature_sizes_ok(res, n) && grid_ok(h, ox, oy, oz, res, n, n),
               "pcgc_feature_combine: bad arguments");
  PCGC_REQUIRE(window_ok(radius, h, &w), "pcgc_feature_combine: radius %g must be positive and below %d cells of edge %g", radius,
               kFeatureMaxWindow, h);
  const CellBuffers b = cell_buffer_layout(res, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_feature_combine: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_cells(b.r, b.keys, b.start, b.bad, Cells{h, ox, oy, oz, res}, kp, n, s, &t);
  if (rc) return rc;
  hipLaunchKernelGGL(feature_combine_kernel, dim3(feature_blocks(n)), dim3(256), 0, s, t, normals, n, w, radius * radius, S, k, feat, valid,
                     b.bad);
  hipLaunchKernelGGL(flag_marks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b.bad, n, valid);
  return launch_ok("feature combine kernels");
}

size_t pcgc_feature_match_workspace_bytes(int64_t n) { return n > 0 && n < 0x7FFFFFFF ? align256((size_t)n * sizeof(unsigned long long)) : 0; }

int pcgc_feature_match(const uint8_t* fs, const uint8_t* vs, int64_t n, const uint8_t* ft, const uint8_t* vt, int64_t m, int32_t* j,
                       uint32_t* dist, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(fs && vs && ft && vt && j && dist && workspace && n > 0 && m > 0 && n < 0x7FFFFFFF && m < 0x7FFFFFFF,
               "pcgc_feature_match: bad arguments");
  PCGC_REQUIRE(((uintptr_t)fs & 3) == 0 && ((uintptr_t)ft & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
               "pcgc_feature_match: the rows must be 4-byte aligned and the workspace 8-byte aligned");
  PCGC_REQUIRE(workspace_bytes >= pcgc_feature_match_workspace_bytes(n), "pcgc_feature_match: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* best = static_cast<unsigned long long*>(workspace);
  PCGC_CHECK_HIP(hipMemsetAsync(best, 0xFF, (size_t)n * sizeof(unsigned long long), s));
  // few source rows: split the target among blockIdx.y so that about a thousand workgroups run
  const int64_t blocks = (n + 255) / 256, tiles = (m + kMatchTile - 1) / kMatchTile;
  const int64_t shares = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(tiles, 1024 / blocks), 65535));
  const int64_t per = (tiles + shares - 1) / shares;
  hipLaunchKernelGGL(feature_match_kernel, dim3((unsigned)blocks, (unsigned)((tiles + per - 1) / per)), dim3(256), 0, s, fs, vs, n, ft, vt,
                     m, per, best);
  hipLaunchKernelGGL(feature_match_final_kernel, dim3((unsigned)blocks), dim3(256), 0, s, best, n, j, dist);
  return launch_ok("feature match kernels");
}

int pcgc_ransac_score(const double* poses, int64_t n_poses, const float* P, const float* Q, int64_t C, double dist, int32_t* counts,
                      pcgc_stream_t stream) {
  PCGC_REQUIRE(poses && P && Q && counts && n_poses > 0 && C > 0 && n_poses < 0x7FFFFFFF && C < 0x7FFFFFFF, "pcgc_ransac_score: bad arguments");
  PCGC_REQUIRE(std::isfinite(dist) && dist > 0.0, "pcgc_ransac_score: dist must be finite and positive (got %g)", dist);
  hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)std::min<int64_t>(n_poses, 16384)), dim3(256), 0, (hipStream_t)stream, poses,
                     n_poses, P, Q, C, dist * dist, counts);
  return launch_ok("ransac score kernel");
}

}  // extern "C"
