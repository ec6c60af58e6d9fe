// The voxel grid the D1 / D2 kernels (tail.hip, offgrid.hip), the colour kernels (color.hip) and the mesh kernels (mesh.hip) share:
// a cloud of integer points < res per axis as an occupancy bit set over res^3 cells, bit (x*res + y)*res + z of a flat
// array of 32-bit words (the cell's linear key: ascending keys are np.unique's lexicographic order).  One copy each of
//   * addressing: cell_of, in_grid, bit_at, and the two kernels that fill a zeroed bit set;
//   * nearest_d2: the exact squared distance to the nearest occupied cell, by Chebyshev shells;
//   * for_each_at_distance: every occupied cell at that distance, in a fixed order (the callers' float sums follow it);
//   * the popcount scan that turns a bit set into per-block offsets of its set bits in key order, and for_each_set_bit,
//     which lists them, and for_each_in_run, the set bits of a z-run of one column;
//   * the rank table over that scan: an occupied cell's index among the set bits (rank_of, build_rank);
//   * find_sorted_key: lower bound in a sorted key list.
// Everything here has internal linkage: the objects link into one library.
#pragma once
#include <algorithm>
#include "common.h"
#include "workspace.h"

namespace pcgc {
namespace {

// ---------------------------------------------------------------------------------------------------------------- addressing
__device__ __forceinline__ int64_t cell_of(int res, int x, int y, int z) { return ((int64_t)x * res + y) * res + z; }

__device__ __forceinline__ bool in_grid(int res, int x, int y, int z) {
  return (unsigned)x < (unsigned)res && (unsigned)y < (unsigned)res && (unsigned)z < (unsigned)res;
}

// false outside the grid
__device__ __forceinline__ bool bit_at(const unsigned* bits, int res, int x, int y, int z) {
  if (!in_grid(res, x, y, z)) return false;
  const int64_t idx = cell_of(res, x, y, z);
  return (bits[idx >> 5] >> (idx & 31)) & 1u;
}

__device__ __forceinline__ void set_bit(unsigned* bits, int64_t idx) { atomicOr(&bits[idx >> 5], 1u << (idx & 31)); }

// one thread per point (int32 x, y, z) or per linear key; what lies outside the grid sets nothing
__global__ void __launch_bounds__(256) bits_from_points_kernel(const int32_t* p, int64_t n, int res, unsigned* bits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  if (in_grid(res, x, y, z)) set_bit(bits, cell_of(res, x, y, z));
}

__global__ void __launch_bounds__(256) bits_from_keys_kernel(const int64_t* keys, int64_t n, int64_t cells, unsigned* bits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t idx = keys[i];
  if (idx >= 0 && idx < cells) set_bit(bits, idx);
}

// ---------------------------------------------------------------------------------------------------------------- search
constexpr unsigned kNoCell = 0xFFFFFFFFu;

// Squared distance from (x, y, z) to the nearest occupied cell; kNoCell when 2 res shells hold none (an empty set: the
// callers that can meet one skip the walk).  Shell w is the surface of the cube of half-width w; after it every unvisited
// cell is farther than w, so the search stops as soon as best <= (w+1)^2.  Exact; typical reconstructions need w <= 2.
__device__ __forceinline__ unsigned nearest_d2(const unsigned* bits, int res, int x, int y, int z) {
  unsigned best = kNoCell;
  for (int w = 0; w < 2 * res; ++w) {
    for (int dx = -w; dx <= w; ++dx)
      for (int dy = -w; dy <= w; ++dy) {
        const bool edge = (dx == -w || dx == w || dy == -w || dy == w);
        const unsigned dxy = (unsigned)(dx * dx + dy * dy);
        if (dxy >= best) continue;
        if (edge) {
          for (int dz = -w; dz <= w; ++dz)
            if (bit_at(bits, res, x + dx, y + dy, z + dz)) best = min(best, dxy + (unsigned)(dz * dz));
        } else {
          if (bit_at(bits, res, x + dx, y + dy, z - w)) best = min(best, dxy + (unsigned)(w * w));
          if (bit_at(bits, res, x + dx, y + dy, z + w)) best = min(best, dxy + (unsigned)(w * w));
        }
      }
    if (best <= (unsigned)((w + 1) * (w + 1))) break;
  }
  return best;
}

// Calls f(dx, dy, qz) for every occupied cell (x + dx, y + dy, qz) at squared distance `best` from (x, y, z): ties are
// kept.  Order: dx ascending, dy ascending, then z + dz before z - dz.  `best` is what nearest_d2 found, not kNoCell.
template <typename F>
__device__ __forceinline__ void for_each_at_distance(const unsigned* bits, int res, int x, int y, int z, unsigned best, F f) {
  const int r = (int)sqrtf((float)best) + 1;
  for (int dx = -r; dx <= r; ++dx)
    for (int dy = -r; dy <= r; ++dy) {
      const int rest = (int)best - dx * dx - dy * dy;
      if (rest < 0) continue;
      int dz = (int)sqrtf((float)rest);
      while (dz * dz > rest) --dz;
      while ((dz + 1) * (dz + 1) <= rest) ++dz;
      if (dz * dz != rest) continue;
      for (int sgn = 0; sgn < (dz ? 2 : 1); ++sgn) {
        const int qz = sgn ? z - dz : z + dz;
        if (bit_at(bits, res, x + dx, y + dy, qz)) f(dx, dy, qz);
      }
    }
}

// first index whose key is not below `key` (n when there is none)
__device__ __forceinline__ int64_t find_sorted_key(const int64_t* keys, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------- popcount scan
// A bit set that is scanned is padded to a whole number of scan blocks (kScanWords words each) and zeroed, so the scan
// reads no bound.  grid_count_kernel, then grid_block_scan_kernel, leave in block_count[b] the number of set bits before
// scan block b; a consumer adds block_scan of its threads' popcounts to reach every word (color.hip's rank table,
// mesh.hip's compaction).
constexpr int kScanThreads = 256, kWordsPerThread = 16, kScanWords = kScanThreads * kWordsPerThread;

// the calling thread's words of scan block blk; returns their popcount
__device__ __forceinline__ unsigned load_words(const unsigned* bits, int64_t blk, unsigned w[kWordsPerThread]) {
  const uint4* src = reinterpret_cast<const uint4*>(bits + blk * kScanWords + (int64_t)threadIdx.x * kWordsPerThread);
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < kWordsPerThread / 4; ++k) {
    const uint4 u = src[k];
    w[4 * k] = u.x; w[4 * k + 1] = u.y; w[4 * k + 2] = u.z; w[4 * k + 3] = u.w;
    c += __popc(u.x) + __popc(u.y) + __popc(u.z) + __popc(u.w);
  }
  return c;
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the workgroup total
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* total) {
  __shared__ unsigned wsum[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanThreads / 64; ++k) {
    before += k < wave ? wsum[k] : 0u;
    all += wsum[k];
  }
  *total = all;
  return before + incl - v;
}

__global__ void __launch_bounds__(kScanThreads) grid_count_kernel(const unsigned* bits, int64_t* block_count) {
  unsigned w[kWordsPerThread];
  const unsigned c = load_words(bits, blockIdx.x, w);
  unsigned total;
  block_scan(c, &total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// exclusive prefix of the per-block counts in place, the sum in *n_set: one workgroup, each thread a contiguous run
__global__ void __launch_bounds__(1024) grid_block_scan_kernel(int64_t* block_count, int64_t nblk, int64_t* n_set) {
  __shared__ int64_t part[1024];
  const int64_t per = (nblk + 1023) / 1024;
  const int64_t b0 = std::min<int64_t>(nblk, (int64_t)threadIdx.x * per), b1 = std::min<int64_t>(nblk, b0 + per);
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += block_count[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc = 0;
    for (int t = 0; t < 1024; ++t) { const int64_t x = part[t]; part[t] = acc; acc += x; }
    *n_set = acc;
  }
  __syncthreads();
  int64_t acc = part[threadIdx.x];
  for (int64_t b = b0; b < b1; ++b) { const int64_t x = block_count[b]; block_count[b] = acc; acc += x; }
}

// f(o, key) for every set bit among the calling thread's words of scan block blockIdx.x, ascending: key = the cell, o = its
// index among all set bits in key order.  A kernel over scan_blocks workgroups of kScanThreads threads, all of them calling,
// lists a bit set this way (mesh.hip's cells and keys, ingest.hip's merged rows).
template <typename F>
__device__ __forceinline__ void for_each_set_bit(const unsigned* bits, const int64_t* block_offset, F f) {
  unsigned w[kWordsPerThread];
  const unsigned c = load_words(bits, blockIdx.x, w);
  unsigned total;
  int64_t o = block_offset[blockIdx.x] + block_scan(c, &total);
  if (c == 0) return;
  const int64_t word0 = (int64_t)blockIdx.x * kScanWords + (int64_t)threadIdx.x * kWordsPerThread;
  for (int k = 0; k < kWordsPerThread; ++k) {
    unsigned x = w[k];
    while (x) {
      const int b = __ffs(x) - 1;
      x &= x - 1;
      f(o, (word0 + k) * 32 + b);
      ++o;
    }
  }
}

// f(w, all, b) for every set bit among bits b0 .. b1 of the set, ascending: bit b of word w, `all` that whole word (the bit's rank
// is rank[w] + popc(all & ((1u << b) - 1u))).  The z-run of a column is cell_of(res, x, y, z0) .. cell_of(res, x, y, z1), z inside
// the row; with res < 32 its words hold other rows too, which the masks drop.
template <typename F>
__device__ __forceinline__ void for_each_in_run(const unsigned* bits, int64_t b0, int64_t b1, F f) {
  for (int64_t w = b0 >> 5; w <= (b1 >> 5); ++w) {
    const int64_t wbit = w << 5;
    const unsigned all = bits[w];
    unsigned word = all;
    if (wbit < b0) word &= ~0u << (int)(b0 - wbit);
    if (wbit + 31 > b1) word &= ~0u >> (int)(wbit + 31 - b1);
    while (word) {
      const int b = __ffs(word) - 1;
      word &= word - 1;
      f(w, all, b);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- rank table
// rank[w] = number of set bits in words 0 .. w-1, one 32-bit entry per word of the padded bit set: the index of an occupied
// cell among the set bits in key order is two loads, no search (color.hip's colours, offgrid.hip's cell starts).
__device__ __forceinline__ int64_t rank_of(const unsigned* bits, const unsigned* rank, int64_t idx) {
  const int64_t w = idx >> 5;
  return (int64_t)rank[w] + __popc(bits[w] & ((1u << (idx & 31)) - 1u));
}

// rank[w] of every word, from the per-block offsets the scan above left
__global__ void __launch_bounds__(kScanThreads) rank_write_kernel(const unsigned* bits, const int64_t* block_offset, unsigned* rank) {
  unsigned w[kWordsPerThread];
  const unsigned c = load_words(bits, blockIdx.x, w);
  unsigned total;
  unsigned o = (unsigned)block_offset[blockIdx.x] + block_scan(c, &total);
  uint4* dst = reinterpret_cast<uint4*>(rank + (int64_t)blockIdx.x * kScanWords + (int64_t)threadIdx.x * kWordsPerThread);
#pragma unroll
  for (int k = 0; k < kWordsPerThread / 4; ++k) {
    uint4 r;
    r.x = o; o += __popc(w[4 * k]);
    r.y = o; o += __popc(w[4 * k + 1]);
    r.z = o; o += __popc(w[4 * k + 2]);
    r.w = o; o += __popc(w[4 * k + 3]);
    dst[k] = r;
  }
}

// host side: scan blocks of a grid of `cells` cells, words of its padded bit set
int64_t scan_blocks(int64_t cells) { return (cells + (int64_t)kScanWords * 32 - 1) / ((int64_t)kScanWords * 32); }

size_t padded_bits_words(int64_t nblk) { return (size_t)nblk * kScanWords; }
size_t padded_bits_bytes(int64_t nblk) { return padded_bits_words(nblk) * sizeof(unsigned); }

// the rank structure of a res^3 grid, and the carver that goes on behind it: a layout that begins with (or holds) a rank
// structure takes its own regions from `rest` (workspace.h: one layout function; null base = size)
struct RankBuffers {
  unsigned* bits;
  unsigned* rank;
  int64_t* block_count;
  int64_t* n_set;
  Carver rest;
};

RankBuffers rank_layout(int res, Carver c) {
  const int64_t nblk = scan_blocks((int64_t)res * res * res);
  RankBuffers r;
  r.bits = c.take<unsigned>(padded_bits_words(nblk));
  r.rank = c.take<unsigned>(padded_bits_words(nblk));
  r.block_count = c.take<int64_t>((size_t)nblk);
  r.n_set = c.take<int64_t>(1);
  r.rest = c;
  return r;
}

// bit set of a cloud given as points (keys == NULL) or as linear keys, and its rank structure
int build_rank(const RankBuffers& r, int res, const int32_t* points, const int64_t* keys, int64_t n, hipStream_t s) {
  const int64_t nblk = scan_blocks((int64_t)res * res * res);
  PCGC_CHECK_HIP(hipMemsetAsync(r.bits, 0, padded_bits_bytes(nblk), s));
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (keys)
    hipLaunchKernelGGL(bits_from_keys_kernel, dim3(grid), dim3(256), 0, s, keys, n, (int64_t)res * res * res, r.bits);
  else
    hipLaunchKernelGGL(bits_from_points_kernel, dim3(grid), dim3(256), 0, s, points, n, res, r.bits);
  hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)nblk), dim3(kScanThreads), 0, s, r.bits, r.block_count);
  hipLaunchKernelGGL(grid_block_scan_kernel, dim3(1), dim3(1024), 0, s, r.block_count, nblk, r.n_set);
  hipLaunchKernelGGL(rank_write_kernel, dim3((unsigned)nblk), dim3(kScanThreads), 0, s, r.bits, r.block_count, r.rank);
  return 0;
}

}  // namespace
}  // namespace pcgc
