// Neighbourhood statistics of a voxel cloud (gfx950): what pcgcv1_amd/clean.py filters outlier voxels of a raw scan on.
//
// include/pcgc.h states the rule (tests/_clean_ref.py restates it in numpy).  For a voxel p, over the occupied
// cells q != p inside the Euclidean ball d2(p, q) <= R^2: cnt = their number, S = the sum of isqrt16(d2) over the k nearest,
// every one of the k that the ball does not hold charged (R + 1) << 16.  isqrt16(d) = floor(sqrt(d * 2^32)) comes from a
// table of R_max^2 + 1 entries that the compiler fills with integer arithmetic; nothing here is floating point, and what is
// added is an integer, so no output depends on the order of the rows or of the threads.
//
// One wave per voxel.  The cloud is the occupancy bit set of voxel_grid.h, z the fastest axis of a cell's key: a lane takes
// columns (dx, dy) of the ball, loads the one to three 32-bit words that cover the column's z-run clipped to the grid, and
// adds every set bit to the wave's histogram over d2 in LDS.  A prefix over the histogram (block_scan, made relative to the
// wave) tells each bin how many of the k nearest it holds.  The whole ball is walked, also when only S is asked for.
#include <algorithm>
#include "common.h"
#include "voxel_grid.h"

namespace pcgc {
namespace {

constexpr int kCleanMaxBits = 12, kCleanMaxK = 64, kCleanMaxR = 32;
constexpr int kCleanBins = kCleanMaxR * kCleanMaxR + 1;        // d2 = 0 .. 1024
constexpr int kCleanWaves = kScanThreads / 64;                 // voxels per workgroup: block_scan wants kScanThreads threads
constexpr int kColumnShift = 20;

// isqrt16(d) = floor(sqrt(d << 32)) for d = 0 .. 1024, by bisection on 64-bit integers at compile time
struct Isqrt16Table {
  uint32_t v[kCleanBins];
  constexpr Isqrt16Table() : v() {
    for (int d = 0; d < kCleanBins; ++d) {
      const uint64_t t = (uint64_t)d << 32;
      uint64_t lo = 0, hi = (uint64_t)(kCleanMaxR + 1) << 16;    // lo^2 <= t < hi^2
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (mid * mid <= t) lo = mid; else hi = mid;
      }
      v[d] = (uint32_t)lo;
    }
  }
};
__device__ const Isqrt16Table kIsqrt16 = Isqrt16Table();

// floor(sqrt(v)) for 0 <= v <= 1024 + 63, bit by bit
__device__ __forceinline__ int isqrt_small(int v) {
  int r = 0;
#pragma unroll
  for (int b = 32; b; b >>= 1) {
    const int t = r + b;
    if (t * t <= v) r = t;
  }
  return r;
}

// S (or NULL) and cnt (or NULL) of voxel blockIdx.x * kCleanWaves + wave.  column_magic = ceil(2^20 / (2 R + 1)): see
// pcgc_clean_neighbors.  No wave leaves before the last barrier.
__global__ void __launch_bounds__(kScanThreads) clean_neighbors_kernel(const int32_t* p, int64_t n, int res, const unsigned* bits, int k,
                                                                       int R, unsigned column_magic, int64_t* S, int32_t* cnt) {
  __shared__ unsigned hist[kCleanWaves][kCleanBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kCleanWaves + wave;
  const int r2 = R * R, nbins = r2 + 1;
  unsigned* h = hist[wave];
  for (int b = lane; b < nbins; b += 64) h[b] = 0;
  __syncthreads();
  int x = -1, y = -1, z = -1;                                   // a voxel outside the grid walks nothing: cnt = 0
  if (i < n) { x = p[i * 3]; y = p[i * 3 + 1]; z = p[i * 3 + 2]; }
  if (in_grid(res, x, y, z)) {
    const int side = 2 * R + 1, columns = side * side;
    for (int c = lane; c < columns; c += 64) {
      const int cx = (int)(((unsigned)c * column_magic) >> kColumnShift);     // c / side
      const int dx = cx - R, dy = c - cx * side - R;
      const int dxy = dx * dx + dy * dy;
      const int qx = x + dx, qy = y + dy;
      if (dxy > r2 || (unsigned)qx >= (unsigned)res || (unsigned)qy >= (unsigned)res) continue;
      const int hz = isqrt_small(r2 - dxy);
      const int64_t row = cell_of(res, qx, qy, 0);
      // the z-run, inside the row
      for_each_in_run(bits, row + max(z - hz, 0), row + min(z + hz, res - 1), [&](int64_t w, unsigned, int b) {
        const int dz = (int)((w << 5) + b - row) - z;
        const int d2 = dxy + dz * dz;                            // <= r2: |dz| <= hz
        if (d2) atomicAdd(&h[d2], 1u);                           // 0: the voxel itself
      });
    }
  }
  __syncthreads();
  // lane l owns the bins [l * per, (l + 1) * per): how many neighbours lie in nearer bins, then its share of the k nearest
  const int per = (nbins + 63) / 64, first = lane * per, last = min(first + per, nbins);
  unsigned mine = 0;
  for (int b = first; b < last; ++b) mine += h[b];
  unsigned total;
  const unsigned upto = block_scan(mine, &total);               // over the workgroup's four voxels, in thread order
  unsigned before = upto - __shfl(upto, 0);                      // within this wave's voxel
  const unsigned count = __shfl(before + mine, 63);
  unsigned sum = 0;                                              // <= 64 * (32 << 16)
  for (int b = first; b < last && before < (unsigned)k; ++b) {
    const unsigned here = h[b];
    sum += min(here, (unsigned)k - before) * kIsqrt16.v[b];
    before += here;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0 && i < n) {
    const unsigned found = min(count, (unsigned)k);
    if (S) S[i] = (int64_t)sum + (int64_t)((unsigned)k - found) * ((int64_t)(R + 1) << 16);
    if (cnt) cnt[i] = (int32_t)count;
  }
}

bool clean_size_ok(int bits, int64_t n) { return bits >= 1 && bits <= kCleanMaxBits && n >= 1 && n <= 0x7FFFFFFF; }

struct CleanBuffers { unsigned* occupied; int64_t nblk; size_t bytes; };     // the occupancy bit set alone, its scan blocks

CleanBuffers clean_layout(int bits, void* workspace) {
  const int res = 1 << bits;
  const int64_t nblk = scan_blocks((int64_t)res * res * res);
  Carver c(workspace);
  unsigned* occupied = c.take<unsigned>(padded_bits_words(nblk));
  return {occupied, nblk, c.bytes()};
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_clean_workspace_bytes(int bits, int64_t n) { return clean_size_ok(bits, n) ? clean_layout(bits, nullptr).bytes : 0; }

int pcgc_clean_neighbors(const int32_t* points, int64_t n, int bits, int k, int radius, int64_t* S, int32_t* cnt, void* workspace,
                         size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && workspace && clean_size_ok(bits, n), "pcgc_clean_neighbors: bad arguments");
  PCGC_REQUIRE(k >= 0 && k <= kCleanMaxK, "pcgc_clean_neighbors: k = %d outside 0..%d", k, kCleanMaxK);
  PCGC_REQUIRE(radius >= 1 && radius <= kCleanMaxR, "pcgc_clean_neighbors: radius = %d outside 1..%d", radius, kCleanMaxR);
  PCGC_REQUIRE(S || cnt, "pcgc_clean_neighbors: neither S nor cnt is asked for");
  PCGC_REQUIRE(k > 0 || !S, "pcgc_clean_neighbors: S with k = 0");
  const CleanBuffers b = clean_layout(bits, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_clean_neighbors: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int res = 1 << bits;
  PCGC_CHECK_HIP(hipMemsetAsync(b.occupied, 0, padded_bits_bytes(b.nblk), s));
  hipLaunchKernelGGL(bits_from_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, res, b.occupied);
  // column c of the (2R+1)^2 square is (c / side, c % side), the quotient as (c * magic) >> 20 with magic = ceil(2^20 / side):
  // magic = 2^20 / side + e with 0 <= e < 1, so the product exceeds the exact c * 2^20 / side by c * e < side^2 <= 4225; the
  // exact value lies at least 2^20 / side >= 16131 below the next multiple of 2^20, so the shift gives c / side.  c * magic < 2^27
  const unsigned side = 2 * (unsigned)radius + 1, magic = ((1u << kColumnShift) + side - 1) / side;
  hipLaunchKernelGGL(clean_neighbors_kernel, dim3((unsigned)((n + kCleanWaves - 1) / kCleanWaves)), dim3(kScanThreads), 0, s, points, n,
                     res, b.occupied, k, radius, magic, S, cnt);
  return launch_ok("clean neighbour kernels");
}

}  // extern "C"
