// The dominant plane of a voxel cloud (gfx950): what pcgcv1_amd/clean.py scores its RANSAC draws with and drops a floor or a
// table by.
//
// include/pcgc.h states the rule (tests/_plane_ref.py restates it in numpy).  A plane is five int64 numbers
// (a, b, c, d, T) and a voxel is an inlier when |a x + b y + c z - d| <= T.  Both kernels test it in one form: with
//   u = a x + b y + c z + (T - d)  as a uint64 (wrapping),   lim = T < 0 ? 0 : 2 T + 1,
// the voxel is an inlier when u < lim.  Inside the stated bounds nothing wraps and this is the rule (a negative s + T has its
// top bit set and lim < 2^55); outside them the sums wrap, the answer is unspecified and no address depends on it.
//
//   * plane_count_kernel   kPlanePointTile = 2048 points per workgroup (256 threads, kPlanePerLane = 8 points per lane, held
//     in vector registers) against kPlaneChunk = 64 planes per workgroup; the grid is (point tiles, plane chunks).  The
//     plane index is the same for a whole wave, so its five words come by uniform loads and the per-plane work (T - d, lim,
//     the width test below) is scalar.  A plane whose a, b, c fit int32 (every draw does) takes three 32 x 32 -> 64
//     multiply-adds per point, any other (a refit plane) the 64-bit products; the choice is per plane, on the device, so the
//     call reads nothing back.  The comparison's lane mask is the ballot: a population count per point slot, summed in
//     scalar registers, is the wave's count of plane j, which lane j of the wave keeps.  After the chunk the four waves add
//     their lanes into 64 LDS words and the workgroup adds each non-zero word to counts[h] with one atomic.
//   * plane_select_kernel  one pass, a point per thread in a grid-stride loop: the mask byte, and with `sums` ten int64
//     accumulators per lane (N, the three coordinates, their squares, xy, xz, yz), reduced over the wave by shuffles, over the
//     workgroup through LDS and added by ten 64-bit atomics per workgroup.  Always the 64-bit products.
// Integer atomics only: neither result depends on the order of the rows or of the threads, and two calls give the same bytes.
// No wave leaves before the last barrier of its kernel.
#include "common.h"

namespace pcgc {
namespace {

constexpr int kPlaneMaxBits = 12;
constexpr int64_t kPlaneMaxK = 65536;
constexpr int kPlaneThreads = 256;
constexpr int kPlanePerLane = 8;
constexpr int kPlanePointTile = kPlaneThreads * kPlanePerLane;      // 2048 points per workgroup
constexpr int kPlaneChunk = 64;                                     // planes per workgroup: one per lane of a wave
constexpr int kSelectThreads = 256, kSelectWaves = kSelectThreads / 64;
constexpr int kSelectMaxBlocks = 2048;
constexpr int kPlaneSums = 10;

struct PlaneTest {
  uint64_t a, b, c, e, lim;      // e = T - d
};

__device__ __forceinline__ PlaneTest load_plane(const int64_t* __restrict__ plane) {
  PlaneTest t;
  t.a = (uint64_t)plane[0];
  t.b = (uint64_t)plane[1];
  t.c = (uint64_t)plane[2];
  const uint64_t T = (uint64_t)plane[4];
  t.e = T - (uint64_t)plane[3];
  t.lim = plane[4] < 0 ? 0 : 2 * T + 1;
  return t;
}

__device__ __forceinline__ bool fits_int32(uint64_t v) { return (int64_t)v == (int64_t)(int32_t)v; }

// x, y, z are inside the grid: 0 .. 4095
__device__ __forceinline__ uint64_t plane_u_wide(const PlaneTest& t, int x, int y, int z) {
  return t.a * (uint64_t)(uint32_t)x + t.b * (uint64_t)(uint32_t)y + t.c * (uint64_t)(uint32_t)z + t.e;
}

__device__ __forceinline__ uint64_t plane_u_narrow(int a, int b, int c, uint64_t e, int x, int y, int z) {
  return (uint64_t)((int64_t)a * x) + (uint64_t)((int64_t)b * y) + (uint64_t)((int64_t)c * z) + e;
}

__global__ void __launch_bounds__(kPlaneThreads) plane_count_kernel(const int32_t* __restrict__ points, int64_t n, int res,
                                                                    const int64_t* __restrict__ planes, int64_t K,
                                                                    int32_t* __restrict__ counts) {
  __shared__ unsigned wg_count[kPlaneChunk];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < kPlaneChunk) wg_count[threadIdx.x] = 0;
  int x[kPlanePerLane], y[kPlanePerLane], z[kPlanePerLane];
  unsigned long long live[kPlanePerLane];                           // per point slot: the lanes whose point is inside the grid
  const int64_t first = (int64_t)blockIdx.x * kPlanePointTile + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kPlanePerLane; ++k) {
    const int64_t i = first + (int64_t)k * kPlaneThreads;
    bool ok = false;
    x[k] = y[k] = z[k] = 0;
    if (i < n) {
      const int px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
      ok = (unsigned)px < (unsigned)res && (unsigned)py < (unsigned)res && (unsigned)pz < (unsigned)res;
      if (ok) { x[k] = px; y[k] = py; z[k] = pz; }
    }
    live[k] = __ballot(ok);
  }
  const int64_t h0 = (int64_t)blockIdx.y * kPlaneChunk;
  const int chunk = (int)(K - h0 < kPlaneChunk ? K - h0 : kPlaneChunk);
  unsigned mine = 0;                                                // lane j: this wave's count of plane h0 + j
  for (int j = 0; j < chunk; ++j) {
    const PlaneTest t = load_plane(planes + (h0 + j) * 5);
    unsigned c = 0;
    if (fits_int32(t.a) && fits_int32(t.b) && fits_int32(t.c)) {
      // through readfirstlane (the values are uniform anyway) so that the compiler does not put the 64-bit words it has just
      // compared back in their place and multiply 64 x 64 after all
      const int a32 = __builtin_amdgcn_readfirstlane((int)t.a), b32 = __builtin_amdgcn_readfirstlane((int)t.b),
                c32 = __builtin_amdgcn_readfirstlane((int)t.c);
#pragma unroll
      for (int k = 0; k < kPlanePerLane; ++k)
        c += (unsigned)__popcll(__ballot(plane_u_narrow(a32, b32, c32, t.e, x[k], y[k], z[k]) < t.lim) & live[k]);
    } else {
#pragma unroll
      for (int k = 0; k < kPlanePerLane; ++k) c += (unsigned)__popcll(__ballot(plane_u_wide(t, x[k], y[k], z[k]) < t.lim) & live[k]);
    }
    if (lane == j) mine = c;
  }
  __syncthreads();                                                  // wg_count is zero
  if (mine) atomicAdd(&wg_count[lane], mine);
  __syncthreads();
  if ((int)threadIdx.x < chunk && wg_count[threadIdx.x]) atomicAdd(&counts[h0 + threadIdx.x], (int32_t)wg_count[threadIdx.x]);
}

__global__ void __launch_bounds__(kSelectThreads) plane_select_kernel(const int32_t* __restrict__ points, int64_t n, int res,
                                                                      const int64_t* __restrict__ plane, uint8_t* __restrict__ mask,
                                                                      unsigned long long* __restrict__ sums) {
  __shared__ long long wave_sum[kSelectWaves][kPlaneSums];
  const PlaneTest t = load_plane(plane);
  long long acc[kPlaneSums];
#pragma unroll
  for (int q = 0; q < kPlaneSums; ++q) acc[q] = 0;
  for (int64_t i = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSelectThreads) {
    const int px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
    bool in = (unsigned)px < (unsigned)res && (unsigned)py < (unsigned)res && (unsigned)pz < (unsigned)res;
    if (in) in = plane_u_wide(t, px, py, pz) < t.lim;
    mask[i] = in ? 1 : 0;
    if (in) {
      const long long X = px, Y = py, Z = pz;
      acc[0] += 1;
      acc[1] += X; acc[2] += Y; acc[3] += Z;
      acc[4] += X * X; acc[5] += Y * Y; acc[6] += Z * Z;
      acc[7] += X * Y; acc[8] += X * Z; acc[9] += Y * Z;
    }
  }
  if (!sums) return;                                                // the same for every thread of the grid
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kPlaneSums; ++q) {
    long long v = acc[q];
    for (int step = 32; step; step >>= 1) v += __shfl_xor(v, step);
    if (lane == 0) wave_sum[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < kPlaneSums) {
    long long v = 0;
    for (int w = 0; w < kSelectWaves; ++w) v += wave_sum[w][threadIdx.x];
    if (v) atomicAdd(&sums[threadIdx.x], (unsigned long long)v);
  }
}

bool plane_size_ok(int bits, int64_t n) { return bits >= 1 && bits <= kPlaneMaxBits && n >= 1 && n <= 0x7FFFFFFF; }

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_plane_count(const int32_t* points, int64_t n, int bits, const int64_t* planes, int64_t K, int32_t* counts, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && planes && counts && plane_size_ok(bits, n), "pcgc_plane_count: bad arguments");
  PCGC_REQUIRE(K >= 1 && K <= kPlaneMaxK, "pcgc_plane_count: K = %lld outside 1..%lld", (long long)K, (long long)kPlaneMaxK);
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int32_t), s));
  const dim3 grid((unsigned)((n + kPlanePointTile - 1) / kPlanePointTile), (unsigned)((K + kPlaneChunk - 1) / kPlaneChunk));
  hipLaunchKernelGGL(plane_count_kernel, grid, dim3(kPlaneThreads), 0, s, points, n, 1 << bits, planes, K, counts);
  return launch_ok("plane_count_kernel");
}

int pcgc_plane_select(const int32_t* points, int64_t n, int bits, const int64_t* plane, uint8_t* mask, int64_t* sums, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && plane && mask && plane_size_ok(bits, n), "pcgc_plane_select: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (sums) PCGC_CHECK_HIP(hipMemsetAsync(sums, 0, kPlaneSums * sizeof(int64_t), s));
  const int64_t blocks = (n + kSelectThreads - 1) / kSelectThreads;
  hipLaunchKernelGGL(plane_select_kernel, dim3((unsigned)(blocks < kSelectMaxBlocks ? blocks : kSelectMaxBlocks)), dim3(kSelectThreads), 0, s,
                     points, n, 1 << bits, plane, mask, reinterpret_cast<unsigned long long*>(sums));
  return launch_ok("plane_select_kernel");
}

}  // extern "C"
