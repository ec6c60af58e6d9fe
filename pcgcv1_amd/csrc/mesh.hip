// Mesh -> point cloud with normals (gfx950): the data preparation of dataprocess/mesh2pc_open3d.py:55-85.
//
//   mesh2pc_open3d.py:57-63   read_triangle_mesh + sample_points_uniformly   -> mesh_sample_kernel
//   mesh2pc_open3d.py:64-67   np.dot(points, get_rotate_matrix())            -> mesh_sample_kernel
//   mesh2pc_open3d.py:68-73   min / max / round voxelisation, np.unique       -> mesh_minmax_*, mesh_quantize_kernel, bitset scan
//   mesh2pc_open3d.py:75-78   estimate_normals(KDTreeSearchParamHybrid(10, 20)) -> normals_kernel
//
// Every floating-point step of the sampler and the voxeliser is one IEEE double operation in a fixed order (the file is
// built with -ffp-contract=off), so tests/_mesh_ref.py restates them in numpy bit for bit.  Integer sets are formed as
// the occupancy bit set of voxel_grid.h, and np.unique's lexicographic order is the bit order: its two-pass scan over
// per-word popcounts, then bits_compact_kernel here, lists the set bits in linear-key order.
#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>
#include "common.h"
#include "jacobi3.h"
#include "voxel_grid.h"

namespace pcgc {
namespace {

// ---------------------------------------------------------------------------------------------------------------- sampling
__device__ __forceinline__ uint64_t splitmix_out(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// draw k of sample i: the (3 i + k + 1)-th output of splitmix64 seeded with `seed`, as a double in [0, 1)
__device__ __forceinline__ double mesh_uniform(uint64_t seed, int64_t i, int k) {
  const uint64_t h = splitmix_out(seed + (uint64_t)(3 * i + k + 1) * 0x9E3779B97F4A7C15ull);
  return (double)(h >> 11) * 0x1.0p-53;
}

__global__ void __launch_bounds__(256) mesh_sample_kernel(const double* v, const int32_t* tri, const double* cdf, int64_t T,
                                                          int64_t n, uint64_t seed, const double* rot, double* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double u0 = mesh_uniform(seed, i, 0), u1 = mesh_uniform(seed, i, 1), u2 = mesh_uniform(seed, i, 2);
  const double total = cdf[T - 1];
  const double target = u0 * total;
  int64_t lo = 0, hi = T;                        // upper_bound: first t with cdf[t] > target
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] <= target) lo = mid + 1; else hi = mid;
  }
  if (lo == T) {                                 // target rounded up to the total: the last triangle of positive area
    lo = 0; hi = T;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cdf[mid] < total) lo = mid + 1; else hi = mid;
    }
  }
  const int32_t* t = tri + lo * 3;
  const double s = sqrt(u1);
  const double a = 1.0 - s, b = s * (1.0 - u2), c = s * u2;
  double p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ab = a * v[(int64_t)t[0] * 3 + k] + b * v[(int64_t)t[1] * 3 + k];
    p[k] = ab + c * v[(int64_t)t[2] * 3 + k];
  }
  if (rot) {                                     // row vector times m: x'_k = (x m0k + y m1k) + z m2k
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (p[0] * rot[k] + p[1] * rot[3 + k]) + p[2] * rot[6 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = q[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[i * 3 + k] = p[k];
}

// ---------------------------------------------------------------------------------------------------------------- voxelising
constexpr int kMinMaxBlocks = 512;

__global__ void __launch_bounds__(256) mesh_minmax_partial_kernel(const double* p, int64_t m, double* partial) {
  __shared__ double smin[256], smax[256];
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    lo = fmin(lo, p[i]);
    hi = fmax(hi, p[i]);
  }
  smin[threadIdx.x] = lo;
  smax[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + o]);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partial[blockIdx.x * 2] = smin[0]; partial[blockIdx.x * 2 + 1] = smax[0]; }
}

// mm[0] = m = min of all coordinates, mm[1] = M = max of the shifted coordinates.  fl(x - m) is monotone in x, so the
// largest shifted coordinate is fl(max - m): one pass finds both.
__global__ void mesh_minmax_final_kernel(const double* partial, int nb, double* mm) {
  if (threadIdx.x == 0) {
    double lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < nb; ++b) { lo = fmin(lo, partial[b * 2]); hi = fmax(hi, partial[b * 2 + 1]); }
    mm[0] = lo;
    mm[1] = hi - lo;
  }
}

// q = rint((p - m) / M * resolution) (np.round: half to even), one bit per cell of the (resolution + 1)^3 grid
__global__ void __launch_bounds__(256) mesh_quantize_kernel(const double* p, int64_t n, const double* mm, int resolution,
                                                            unsigned* bits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double m = mm[0], M = mm[1];
  const int64_t G = resolution + 1;
  int64_t q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double r = M > 0.0 ? rint((p[i * 3 + k] - m) / M * (double)resolution) : 0.0;   // M == 0: one point, every coordinate 0
    q[k] = (int64_t)r;
    if (!(r >= 0.0 && r <= (double)resolution)) return;                                     // unreachable for finite input
  }
  const int64_t key = (q[0] * G + q[1]) * G + q[2];
  set_bit(bits, key);
}

// ---------------------------------------------------------------------------------------------------------------- bit set scan
// every set bit in key order: voxelize writes the cell's coordinates (int32 x, y, z of the G^3 grid), the normals path
// its key.  Writes stop at cap (the callers size cap to the number of input points, which bounds the set bits).
template <bool kCoords>
__global__ void __launch_bounds__(kScanThreads) bits_compact_kernel(const unsigned* bits, const int64_t* block_offset, int64_t G,
                                                                    int64_t cap, int32_t* coords, int64_t* keys) {
  for_each_set_bit(bits, block_offset, [&](int64_t o, int64_t key) {
    if (o >= cap) return;
    if (kCoords) {
      coords[o * 3] = (int32_t)(key / (G * G));
      coords[o * 3 + 1] = (int32_t)((key / G) % G);
      coords[o * 3 + 2] = (int32_t)(key % G);
    } else {
      keys[o] = key;
    }
  });
}

// ---------------------------------------------------------------------------------------------------------------- normals
// the cyclic Jacobi of the covariance: jacobi3.h
// normal of one occupied cell from its integer neighbour sums (K, S = sum d, Q = sum d d^T); see include/pcgc.h
__device__ void normal_from_sums(int K, const int64_t S[3], const int64_t Q[6], int64_t C[6], float out[3]) {
  // C = K Q - S S^T: c00 c01 c02 c11 c12 c22
  C[0] = K * Q[0] - S[0] * S[0]; C[1] = K * Q[1] - S[0] * S[1]; C[2] = K * Q[2] - S[0] * S[2];
  C[3] = K * Q[3] - S[1] * S[1]; C[4] = K * Q[4] - S[1] * S[2]; C[5] = K * Q[5] - S[2] * S[2];
  double n[3];
  if (K < 3) {
    n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
  } else {
    const int64_t m[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    bool rank_le1 = true;                         // every 2x2 minor zero
    for (int r0 = 0; r0 < 3; ++r0)
      for (int r1 = r0 + 1; r1 < 3; ++r1)
        for (int c0 = 0; c0 < 3; ++c0)
          for (int c1 = c0 + 1; c1 < 3; ++c1)
            rank_le1 = rank_le1 && m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0] == 0;
    if (rank_le1) {
      // collinear neighbours: u = the row of C with the largest diagonal entry, normal = normalize(u x e_j)
      int r = 0;
      for (int k = 1; k < 3; ++k) if (m[k][k] > m[r][r]) r = k;
      const double u[3] = {(double)m[r][0], (double)m[r][1], (double)m[r][2]};
      int j = 0;
      for (int k = 1; k < 3; ++k) if (fabs(u[k]) < fabs(u[j])) j = k;
      if (j == 0) { n[0] = 0.0; n[1] = u[2]; n[2] = -u[1]; }
      else if (j == 1) { n[0] = -u[2]; n[1] = 0.0; n[2] = u[0]; }
      else { n[0] = u[1]; n[1] = -u[0]; n[2] = 0.0; }
    } else {
      double a[3][3], v[3][3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[r][c] = (double)m[r][c];
      jacobi3(a, v);
      const int j = a[1][1] < a[0][0] ? (a[2][2] < a[1][1] ? 2 : 1) : (a[2][2] < a[0][0] ? 2 : 0);
      for (int k = 0; k < 3; ++k) n[k] = j == 0 ? v[k][0] : j == 1 ? v[k][1] : v[k][2];
    }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    for (int k = 0; k < 3; ++k) n[k] /= len;
    for (int k = 0; k < 3; ++k)                   // sign: the first component with |c| > 1e-6 is positive
      if (fabs(n[k]) > 1e-6) {
        if (n[k] < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        break;
      }
  }
  for (int k = 0; k < 3; ++k) out[k] = (float)n[k];
}

// One lane per occupied cell, cells in key order (a wave's probes then share bit-set words).  The lanes of a wave walk
// the offset table together; the table index is wave-uniform, so its entries come through the scalar cache, and the
// wave leaves when every lane has max_nn neighbours or the table ends.
__global__ void __launch_bounds__(256) normals_kernel(const unsigned* bits, const int64_t* ukeys, const int64_t* n_cells, int res,
                                                      const int32_t* table, int n_table, int max_nn, float* unormals,
                                                      int64_t* ucov, int32_t* uk) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nc = *n_cells;
  if ((int64_t)blockIdx.x * 256 >= nc) return;            // whole workgroup past the end (uniform)
  const bool live = i < nc;
  const int64_t key = live ? ukeys[i] : 0;
  const int x = (int)(key / ((int64_t)res * res)), y = (int)((key / res) % res), z = (int)(key % res);
  int K = 0;
  int sx = 0, sy = 0, sz = 0, qxx = 0, qxy = 0, qxz = 0, qyy = 0, qyz = 0, qzz = 0;
  for (int j = 0; j < n_table; ++j) {
    const bool need = live && K < max_nn;
    if (!__any(need)) break;
    const int e = table[j];
    const int dx = (e & 63) - 32, dy = ((e >> 6) & 63) - 32, dz = ((e >> 12) & 63) - 32;
    if (need && bit_at(bits, res, x + dx, y + dy, z + dz)) {
      ++K;
      sx += dx; sy += dy; sz += dz;
      qxx += dx * dx; qxy += dx * dy; qxz += dx * dz; qyy += dy * dy; qyz += dy * dz; qzz += dz * dz;
    }
  }
  if (!live) return;
  const int64_t S[3] = {sx, sy, sz}, Q[6] = {qxx, qxy, qxz, qyy, qyz, qzz};
  int64_t C[6];
  float nrm[3];
  normal_from_sums(K, S, Q, C, nrm);
  for (int k = 0; k < 3; ++k) unormals[i * 3 + k] = nrm[k];
  if (ucov) {
    for (int k = 0; k < 6; ++k) ucov[i * 6 + k] = C[k];
    uk[i] = K;
  }
}

// input order: each point finds its cell among the sorted keys (duplicates share it)
__global__ void __launch_bounds__(256) normals_gather_kernel(const int32_t* p, int64_t n, int res, const int64_t* ukeys,
                                                             const int64_t* n_cells, const float* unormals, const int64_t* ucov,
                                                             const int32_t* uk, float* normals, int64_t* cov, int32_t* nn) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  const int64_t key = cell_of(res, x, y, z);
  const int64_t nc = *n_cells;
  const int64_t lo = find_sorted_key(ukeys, nc, key);
  const bool found = in_grid(res, x, y, z) && lo < nc && ukeys[lo] == key;
  for (int k = 0; k < 3; ++k) normals[i * 3 + k] = found ? unormals[lo * 3 + k] : 0.f;
  if (cov) {
    for (int k = 0; k < 6; ++k) cov[i * 6 + k] = found ? ucov[lo * 6 + k] : 0;
    nn[i] = found ? uk[lo] : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// offsets with dx^2 + dy^2 + dz^2 <= r2, sorted by (d^2, dx, dy, dz), packed as (dx+32) | (dy+32) << 6 | (dz+32) << 12.
// Built once per r2 and kept for the process (the copy to the device reads it asynchronously).
const std::vector<int32_t>& offset_table(int r2) {
  static std::mutex mu;
  static std::map<int, std::vector<int32_t>> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(r2);
  if (it != cache.end()) return it->second;
  int r = 0;
  while ((r + 1) * (r + 1) <= r2) ++r;
  std::vector<std::array<int, 4>> e;
  for (int dx = -r; dx <= r; ++dx)
    for (int dy = -r; dy <= r; ++dy)
      for (int dz = -r; dz <= r; ++dz) {
        const int d2 = dx * dx + dy * dy + dz * dz;
        if (d2 <= r2) e.push_back({d2, dx, dy, dz});
      }
  std::sort(e.begin(), e.end());
  std::vector<int32_t> t(e.size());
  for (size_t k = 0; k < e.size(); ++k) t[k] = (e[k][1] + 32) | ((e[k][2] + 32) << 6) | ((e[k][3] + 32) << 12);
  return cache.emplace(r2, std::move(t)).first->second;
}

int radius2(double radius) { return (int)std::floor(radius * radius); }

// pcgc_mesh_voxelize: the bit set of the (resolution + 1)^3 grid, its scan, the min / max partials and the pair they reduce to
struct VoxelizeBuffers { unsigned* bits; int64_t* block_count; double *partial, *mm; int64_t G, nblk; size_t bytes; };

VoxelizeBuffers voxelize_layout(int resolution, void* workspace) {
  Carver c(workspace);
  VoxelizeBuffers b;
  b.G = resolution + 1;
  b.nblk = scan_blocks(b.G * b.G * b.G);
  b.bits = c.take<unsigned>(padded_bits_words(b.nblk));
  b.block_count = c.take<int64_t>((size_t)b.nblk);
  b.partial = c.take<double>(2 * kMinMaxBlocks);
  b.mm = c.take<double>(2);
  b.bytes = c.bytes();
  return b;
}

// pcgc_estimate_normals: bit set and scan of the res^3 grid, the number of cells, per cell its key, normal, covariance and
// neighbour count, then the offset table of n_table entries
struct NormalsBuffers {
  unsigned* bits; int64_t *block_count, *n_cells, *ukeys; float* unormals; int64_t* ucov; int32_t *uk, *dtable;
  int64_t nblk; size_t bytes;
};

NormalsBuffers normals_layout(int res, int64_t n, size_t n_table, void* workspace) {
  Carver c(workspace);
  NormalsBuffers b;
  b.nblk = scan_blocks((int64_t)res * res * res);
  b.bits = c.take<unsigned>(padded_bits_words(b.nblk));
  b.block_count = c.take<int64_t>((size_t)b.nblk);
  b.n_cells = c.take<int64_t>(1);
  b.ukeys = c.take<int64_t>((size_t)n);
  b.unormals = c.take<float>((size_t)n * 3);
  b.ucov = c.take<int64_t>((size_t)n * 6);
  b.uk = c.take<int32_t>((size_t)n);
  b.dtable = c.take<int32_t>(n_table);
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_mesh_sample(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                     const double* area_cdf, int64_t n_points, uint64_t seed, const double* rotation, double* points,
                     pcgc_stream_t stream) {
  PCGC_REQUIRE(n_points >= 0 && (n_points == 0 || (vertices && n_vertices > 0 && triangles && n_triangles > 0 && area_cdf && points)),
               "pcgc_mesh_sample: bad arguments");
  if (n_points == 0) return 0;
  hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices,
                     triangles, area_cdf, n_triangles, n_points, seed, rotation, points);
  return launch_ok("mesh_sample_kernel");
}

size_t pcgc_mesh_voxelize_workspace_bytes(int resolution) {
  return resolution >= 1 && resolution <= 4095 ? voxelize_layout(resolution, nullptr).bytes : 0;
}

int pcgc_mesh_voxelize(const double* points, int64_t n, int resolution, int32_t* out, int64_t cap, int64_t* n_out,
                       void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && out && n_out && n > 0 && resolution >= 1 && resolution <= 4095 && workspace,
               "pcgc_mesh_voxelize: bad arguments");
  PCGC_REQUIRE(cap >= n, "pcgc_mesh_voxelize: capacity %lld below the %lld input points", (long long)cap, (long long)n);
  const VoxelizeBuffers b = voxelize_layout(resolution, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_mesh_voxelize: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemsetAsync(b.bits, 0, padded_bits_bytes(b.nblk), s));
  const int64_t m = 3 * n;
  const int nb = (int)std::min<int64_t>(kMinMaxBlocks, (m + 255) / 256);
  hipLaunchKernelGGL(mesh_minmax_partial_kernel, dim3(nb), dim3(256), 0, s, points, m, b.partial);
  hipLaunchKernelGGL(mesh_minmax_final_kernel, dim3(1), dim3(64), 0, s, b.partial, nb, b.mm);
  hipLaunchKernelGGL(mesh_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, b.mm, resolution, b.bits);
  hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)b.nblk), dim3(kScanThreads), 0, s, b.bits, b.block_count);
  hipLaunchKernelGGL(grid_block_scan_kernel, dim3(1), dim3(1024), 0, s, b.block_count, b.nblk, n_out);
  hipLaunchKernelGGL(bits_compact_kernel<true>, dim3((unsigned)b.nblk), dim3(kScanThreads), 0, s, b.bits, b.block_count, b.G, cap, out,
                     (int64_t*)nullptr);
  return launch_ok("mesh voxelize kernels");
}

int pcgc_normals_table_size(double radius) {
  if (!(radius >= 0.0 && radius <= 16.0)) return -1;
  return (int)offset_table(radius2(radius)).size();
}

size_t pcgc_normals_workspace_bytes(int res, int64_t n, double radius) {
  if (res < 1 || res > 4096 || n < 0 || !(radius >= 0.0 && radius <= 16.0)) return 0;
  return normals_layout(res, n, offset_table(radius2(radius)).size(), nullptr).bytes;
}

int pcgc_estimate_normals(const int32_t* points, int64_t n, int res, double radius, int max_nn, float* normals, int64_t* cov,
                          int32_t* n_neighbours, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && normals && n > 0 && res >= 1 && res <= 4096 && radius >= 0.0 && radius <= 16.0 && max_nn >= 1 &&
               max_nn <= 64 && workspace && (cov == nullptr) == (n_neighbours == nullptr),
               "pcgc_estimate_normals: bad arguments");
  const std::vector<int32_t>& table = offset_table(radius2(radius));
  const NormalsBuffers b = normals_layout(res, n, table.size(), workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_estimate_normals: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemcpyAsync(b.dtable, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  PCGC_CHECK_HIP(hipMemsetAsync(b.bits, 0, padded_bits_bytes(b.nblk), s));
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(bits_from_points_kernel, dim3(grid), dim3(256), 0, s, points, n, res, b.bits);
  hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)b.nblk), dim3(kScanThreads), 0, s, b.bits, b.block_count);
  hipLaunchKernelGGL(grid_block_scan_kernel, dim3(1), dim3(1024), 0, s, b.block_count, b.nblk, b.n_cells);
  hipLaunchKernelGGL(bits_compact_kernel<false>, dim3((unsigned)b.nblk), dim3(kScanThreads), 0, s, b.bits, b.block_count, (int64_t)res, n,
                     (int32_t*)nullptr, b.ukeys);
  hipLaunchKernelGGL(normals_kernel, dim3(grid), dim3(256), 0, s, b.bits, b.ukeys, b.n_cells, res, b.dtable, (int)table.size(), max_nn,
                     b.unormals, cov ? b.ucov : nullptr, b.uk);
  hipLaunchKernelGGL(normals_gather_kernel, dim3(grid), dim3(256), 0, s, points, n, res, b.ukeys, b.n_cells, b.unormals, b.ucov, b.uk,
                     normals, cov, n_neighbours);
  return launch_ok("normal estimation kernels");
}

}  // extern "C"
