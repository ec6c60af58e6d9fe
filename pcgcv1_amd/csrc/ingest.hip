// Raw scan -> voxel cloud with merged colours and normals (gfx950): the ingest step of pcgcv1_amd/ingest.py.
//
// A scan has float64 coordinates in its own units and any number of points per voxel.  include/pcgc.h states the rule
// (tests/_ingest_ref.py restates it in numpy): bounds over the finite rows, q = floor((p - origin) / step +
// 0.5) clamped to the grid, then one row per occupied voxel in key order with its count, the exact mean of its colours and
// the normalised sum of its normals.  Every position step is one IEEE double operation in the stated order (the file is built
// with -ffp-contract=off and without any fast-math flag: non-finite input is part of the rule).  Everything that is summed
// is an integer, added with integer atomics, so no output depends on the order of the rows or of the threads.
//
// The voxels are the occupancy bit set, popcount scan and rank table of voxel_grid.h: a point's voxel row is rank_of(its
// key); the rows are written by for_each_set_bit.  [n,3] arrays are read through LDS, consecutive lanes loading
// consecutive elements, then each thread takes its own row.
#include <algorithm>
#include <cmath>
#include "common.h"
#include "voxel_grid.h"

namespace pcgc {
namespace {

constexpr int kIngestMaxBits = 12;
constexpr int kBoundsBlocks = 1024;
constexpr double kNormalOne = 1073741824.0;         // 2^30 fixed point for the normal sums
constexpr int64_t kMaxColoredRows = 16843009;       // 2^32 / 255 rounded down: no uint32 colour sum can overflow

// Row (block row0 + threadIdx.x) of an [n,3] array in out[3] (zeros past the end).  Every thread of the 256-thread
// workgroup calls; lds holds 768 elements.
template <typename T>
__device__ __forceinline__ void load_row3(const T* a, int64_t n, int64_t row0, T* lds, T out[3]) {
  const int64_t base = row0 * 3, end = n * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t e = base + k * 256 + threadIdx.x;
    lds[k * 256 + threadIdx.x] = e < end ? a[e] : T(0);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = lds[threadIdx.x * 3 + k];
  __syncthreads();
}

__device__ __forceinline__ bool finite3(const double p[3]) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// ---------------------------------------------------------------------------------------------------------------- bounds
// A double as a uint64 whose unsigned order is the double's order (-inf lowest), so min / max are 64-bit integer atomics:
// order-free, no partial buffers.  -0.0 sorts below +0.0.
__device__ __forceinline__ unsigned long long ordered_of(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double double_of(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// ord[0..2] = ordered(+inf), ord[3..5] = ordered(-inf), *n_dropped = 0
__global__ void ingest_bounds_init_kernel(unsigned long long* ord, int64_t* n_dropped) {
  if (threadIdx.x < 6) ord[threadIdx.x] = ordered_of(threadIdx.x < 3 ? (double)INFINITY : -(double)INFINITY);
  if (threadIdx.x == 6) *n_dropped = 0;
}

__global__ void __launch_bounds__(256) ingest_bounds_kernel(const double* p, int64_t n, unsigned long long* ord, int64_t* n_dropped) {
  __shared__ double rows[768];
  __shared__ double red[6][256];
  __shared__ int dropped[256];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int drop = 0;                                     // < 2^31 rows in all
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    double v[3];
    load_row3(p, n, row0, rows, v);
    if (row0 + threadIdx.x >= n) continue;
    if (!finite3(v)) { ++drop; continue; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], v[k]); hi[k] = fmax(hi[k], v[k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = lo[k]; red[3 + k][threadIdx.x] = hi[k]; }
  dropped[threadIdx.x] = drop;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        red[k][threadIdx.x] = fmin(red[k][threadIdx.x], red[k][threadIdx.x + o]);
        red[3 + k][threadIdx.x] = fmax(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + o]);
      }
      dropped[threadIdx.x] += dropped[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) atomicMin(&ord[threadIdx.x], ordered_of(red[threadIdx.x][0]));
  else if (threadIdx.x < 6) atomicMax(&ord[threadIdx.x], ordered_of(red[threadIdx.x][0]));
  else if (threadIdx.x == 6 && dropped[0]) atomicAdd(reinterpret_cast<unsigned long long*>(n_dropped), (unsigned long long)dropped[0]);
}

// the six ordered keys back to doubles, in place
__global__ void ingest_bounds_final_kernel(unsigned long long* ord) {
  if (threadIdx.x < 6) reinterpret_cast<double*>(ord)[threadIdx.x] = double_of(ord[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------- quantise
struct Frame {
  double ox, oy, oz, step;
  int bits;
};

__global__ void __launch_bounds__(256) ingest_quantize_kernel(const double* p, int64_t n, Frame f, int32_t* q, int64_t* keys) {
  __shared__ double rows[768];
  const int64_t row0 = (int64_t)blockIdx.x * 256, i = row0 + threadIdx.x;
  double v[3];
  load_row3(p, n, row0, rows, v);
  if (i >= n) return;
  int32_t c[3] = {-1, -1, -1};
  int64_t key = -1;
  if (finite3(v)) {
    const double o[3] = {f.ox, f.oy, f.oz}, R = (double)((1 << f.bits) - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double r = floor((v[k] - o[k]) / f.step + 0.5);      // +-inf when the difference overflows, never a NaN
      c[k] = (int32_t)fmin(fmax(r, 0.0), R);
    }
    key = ((((int64_t)c[0]) << f.bits) | c[1]) << f.bits | c[2];
  }
  // three int32 per row, written as they lie: the wave's stores cover one contiguous run
  q[i * 3] = c[0]; q[i * 3 + 1] = c[1]; q[i * 3 + 2] = c[2];
  keys[i] = key;
}

// ---------------------------------------------------------------------------------------------------------------- merge
struct Sums {
  int32_t* count;            // [n]
  uint32_t* color;           // [n,3]
  long long* normal;         // [n,3]
};

// every row adds itself to the accumulators of its voxel's row; a key outside the grid adds nothing
__global__ void __launch_bounds__(256) ingest_accumulate_kernel(const int64_t* keys, int64_t n, int64_t cells, const uint8_t* colors,
                                                                const float* normals, const unsigned* bits, const unsigned* rank,
                                                                Sums s) {
  __shared__ float nrows[768];
  __shared__ uint8_t crows[768];
  const int64_t row0 = (int64_t)blockIdx.x * 256, i = row0 + threadIdx.x;
  uint8_t c[3] = {0, 0, 0};
  float v[3] = {0.f, 0.f, 0.f};
  if (colors) load_row3(colors, n, row0, crows, c);             // uniform branches: the loader synchronises
  if (normals) load_row3(normals, n, row0, nrows, v);
  if (i >= n) return;
  const int64_t key = keys[i];
  if (key < 0 || key >= cells) return;
  const int64_t r = rank_of(bits, rank, key);                    // the key's bit is set: build_rank saw the same keys
  if (r >= n) return;                                           // at most n voxels are occupied
  atomicAdd(&s.count[r], 1);
  if (colors) {
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&s.color[r * 3 + k], (uint32_t)c[k]);
  }
  if (normals) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double d = (double)v[k];
      if (!isfinite(d)) d = 0.0;
      d = fmin(fmax(d, -1.0), 1.0);
      const long long fx = llrint(d * kNormalOne);
      if (fx) atomicAdd(reinterpret_cast<unsigned long long*>(&s.normal[r * 3 + k]), (unsigned long long)fx);
    }
  }
}

// the rows, in key order
__global__ void __launch_bounds__(kScanThreads) ingest_rows_kernel(const unsigned* bits, const int64_t* block_offset, const int64_t* n_set,
                                                                   int bits_per_axis, Sums s, bool with_colors, bool with_normals,
                                                                   int64_t cap, int32_t* out_points, int32_t* out_counts,
                                                                   uint8_t* out_colors, float* out_normals, int64_t* n_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = *n_set;
  const int mask = (1 << bits_per_axis) - 1;
  for_each_set_bit(bits, block_offset, [&](int64_t o, int64_t key) {
    if (o >= cap) return;
    out_points[o * 3] = (int32_t)(key >> (2 * bits_per_axis));
    out_points[o * 3 + 1] = (int32_t)(key >> bits_per_axis) & mask;
    out_points[o * 3 + 2] = (int32_t)key & mask;
    const int32_t count = s.count[o];
    out_counts[o] = count;
    if (with_colors) {
      const uint64_t c2 = 2 * (uint64_t)(uint32_t)count;
#pragma unroll
      for (int k = 0; k < 3; ++k) out_colors[o * 3 + k] = (uint8_t)((2 * (uint64_t)s.color[o * 3 + k] + (uint32_t)count) / c2);
    }
    if (with_normals) {
      const double vx = (double)s.normal[o * 3], vy = (double)s.normal[o * 3 + 1], vz = (double)s.normal[o * 3 + 2];
      const double len = sqrt((vx * vx + vy * vy) + vz * vz);
      out_normals[o * 3] = len == 0.0 ? 0.f : (float)(vx / len);
      out_normals[o * 3 + 1] = len == 0.0 ? 0.f : (float)(vy / len);
      out_normals[o * 3 + 2] = len == 0.0 ? 0.f : (float)(vz / len);
    }
  });
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool ingest_size_ok(int bits, int64_t n) { return bits >= 1 && bits <= kIngestMaxBits && n >= 1 && n <= 0x7FFFFFFF; }

// the rank structure of the grid, then the per-voxel accumulators
struct IngestBuffers { RankBuffers r; Sums sums; size_t bytes; };

IngestBuffers ingest_layout(int bits, int64_t n, void* workspace) {
  IngestBuffers b;
  b.r = rank_layout(1 << bits, workspace);
  Carver& c = b.r.rest;
  b.sums.count = c.take<int32_t>((size_t)n);
  b.sums.color = c.take<uint32_t>((size_t)n * 3);
  b.sums.normal = c.take<long long>((size_t)n * 3);
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_ingest_bounds(const double* points, int64_t n, double* out, int64_t* n_dropped, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && out && n_dropped && n >= 1 && n <= 0x7FFFFFFF, "pcgc_ingest_bounds: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* ord = reinterpret_cast<unsigned long long*>(out);
  const unsigned blocks = (unsigned)std::min<int64_t>(kBoundsBlocks, (n + 255) / 256);
  hipLaunchKernelGGL(ingest_bounds_init_kernel, dim3(1), dim3(64), 0, s, ord, n_dropped);
  hipLaunchKernelGGL(ingest_bounds_kernel, dim3(blocks), dim3(256), 0, s, points, n, ord, n_dropped);
  hipLaunchKernelGGL(ingest_bounds_final_kernel, dim3(1), dim3(64), 0, s, ord);
  return launch_ok("ingest bounds kernels");
}

int pcgc_ingest_quantize(const double* points, int64_t n, const double* origin, double step, int bits, int32_t* q, int64_t* keys,
                         pcgc_stream_t stream) {
  PCGC_REQUIRE(points && origin && q && keys && ingest_size_ok(bits, n), "pcgc_ingest_quantize: bad arguments");
  PCGC_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]) && std::isfinite(step) && step > 0.0,
               "pcgc_ingest_quantize: the origin must be finite and the step finite and positive");
  const Frame f{origin[0], origin[1], origin[2], step, bits};
  hipLaunchKernelGGL(ingest_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, n, f, q, keys);
  return launch_ok("ingest_quantize_kernel");
}

size_t pcgc_ingest_workspace_bytes(int bits, int64_t n) { return ingest_size_ok(bits, n) ? ingest_layout(bits, n, nullptr).bytes : 0; }

int pcgc_ingest_merge(const int64_t* keys, int64_t n, int bits, const uint8_t* colors, const float* normals, int32_t* out_points,
                      int32_t* out_counts, uint8_t* out_colors, float* out_normals, int64_t cap, int64_t* n_out, void* workspace,
                      size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(keys && out_points && out_counts && n_out && workspace && ingest_size_ok(bits, n) && (!colors || out_colors) &&
               (!normals || out_normals), "pcgc_ingest_merge: bad arguments");
  const int res = 1 << bits;
  const int64_t cells = (int64_t)res * res * res, nblk = scan_blocks(cells);
  PCGC_REQUIRE(cap >= std::min(n, cells), "pcgc_ingest_merge: capacity %lld below min(rows, cells) = %lld", (long long)cap,
               (long long)std::min(n, cells));
  PCGC_REQUIRE(!colors || n <= kMaxColoredRows, "pcgc_ingest_merge: %lld rows with colours; the uint32 colour sums hold %lld",
               (long long)n, (long long)kMaxColoredRows);
  const IngestBuffers b = ingest_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_ingest_merge: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const RankBuffers& r = b.r;
  const Sums& sums = b.sums;
  const int rc = build_rank(r, res, nullptr, keys, n, s);       // set bits (keys checked against the grid), scan, rank table
  if (rc) return rc;
  PCGC_CHECK_HIP(hipMemsetAsync(sums.count, 0, (size_t)n * sizeof(int32_t), s));
  if (colors) PCGC_CHECK_HIP(hipMemsetAsync(sums.color, 0, (size_t)n * 3 * sizeof(uint32_t), s));
  if (normals) PCGC_CHECK_HIP(hipMemsetAsync(sums.normal, 0, (size_t)n * 3 * sizeof(long long), s));
  hipLaunchKernelGGL(ingest_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n, cells, colors, normals,
                     r.bits, r.rank, sums);
  hipLaunchKernelGGL(ingest_rows_kernel, dim3((unsigned)nblk), dim3(kScanThreads), 0, s, r.bits, r.block_count, r.n_set, bits, sums,
                     colors != nullptr, normals != nullptr, cap, out_points, out_counts, out_colors, out_normals, n_out);
  return launch_ok("ingest merge kernels");
}

}  // extern "C"
