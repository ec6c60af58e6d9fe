// The exact distance from the points of a cloud to a triangle mesh (gfx950): what pcgcv1_amd/metrics.py: mesh_error measures
// with.  include/pcgc.h states the rule (tests/_mesh_error_ref.py restates it in numpy by brute force); the
// point-triangle function itself is csrc/point_triangle.h, which also compiles on the host.
//
// The triangles are listed in cubic cells of edge h (a power of two) that cover the mesh's bounding box, each triangle in every
// cell its axis-aligned bounding box overlaps.  The cells are the occupancy bit set, the rank table and the cell starts of
// voxel_grid.h and offgrid_cells.h, over (cell key, triangle) pairs instead of points.  torch scans and sorts; the kernels are
//   * meshdist_count_kernel: one thread per triangle, the number of cells its box overlaps;
//   * meshdist_emit_kernel: one thread per triangle, its pairs as words key << 31 | triangle at the offset the scan gave it.
//     One sort of the words orders them by cell and, inside a cell, by ascending triangle;
//   * meshdist_unpack_kernel and meshdist_pack_kernel: the sorted words back into keys and triangles, every one checked, and the
//     nine doubles of every triangle side by side, so that a candidate is 72 contiguous bytes;
//   * meshdist_query_kernel: one thread per point, taken through an optional order (the host sorts the points by cell, so that the
//     lanes of a wave walk the same cells), the Chebyshev shell walk of offgrid.hip's nearest_offgrid with the stopping rule of
//     point_triangle.h; best and nearest are written at the caller's index;
//   * meshdist_reduce_kernel and meshdist_final_kernel: the figures from best[] in the caller's order: per thread in grid-stride
//     order, a fixed tree per workgroup, the workgroups in index order.
// No float atomics: two calls give the same bytes.  Every index read from the caller's arrays is checked before it is used; what
// breaks the contract raises the flag word, and the outputs come back as NaN (nearest as -1).
#include <algorithm>
#include <cmath>
#include "common.h"
#include "offgrid_cells.h"     // Cells, Target, offgrid_starts_kernel, for_each_in_cell, edge_ok, cell_buffer_layout
#include "point_triangle.h"

namespace pcgc {
namespace {

constexpr int kMeshThreads = 256, kMeshBlocks = 1024, kMeshTriBits = 31;
constexpr double kMeshLimit = 1048576.0;            // 2^20: every coordinate lies strictly inside

unsigned mesh_blocks(int64_t n) { return (unsigned)((n + kMeshThreads - 1) / kMeshThreads); }

struct CellBox {
  int lo[3], hi[3];
};

// the corners of triangle t into p[3][3]; false for a corner outside 0..V-1 or a coordinate that is not finite or not below 2^20
__device__ __forceinline__ bool load_triangle(const double* v, int64_t V, const int32_t* tri, int64_t t, double p[3][3]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int32_t i = tri[t * 3 + j];
    const bool inside = i >= 0 && i < V;
    ok = ok && inside;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = inside ? v[(int64_t)i * 3 + k] : 0.0;
      ok = ok && fabs(x) < kMeshLimit;                                 // false for a NaN
      p[j][k] = x;
    }
  }
  return ok;
}

// the cells the bounding box of a triangle overlaps; false where it leaves the grid
__device__ __forceinline__ bool cell_box(const Cells& c, const double p[3][3], CellBox* box) {
  const int origin[3] = {c.ox, c.oy, c.oz};
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = fmin(fmin(p[0][k], p[1][k]), p[2][k]), hi = fmax(fmax(p[0][k], p[1][k]), p[2][k]);
    const double c0 = floor(lo / c.h) - (double)origin[k], c1 = floor(hi / c.h) - (double)origin[k];
    ok = ok && c0 >= 0.0 && c1 < (double)c.res && c0 <= c1;
    box->lo[k] = ok ? (int)c0 : 0;
    box->hi[k] = ok ? (int)c1 : 0;
  }
  return ok;
}

__device__ __forceinline__ int64_t box_cells(const CellBox& b) {
  return (int64_t)(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1) * (b.hi[2] - b.lo[2] + 1);
}

__global__ void __launch_bounds__(kMeshThreads) meshdist_count_kernel(const double* v, int64_t V, const int32_t* tri, int64_t T, Cells c,
                                                                     int64_t* counts, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (t >= T) return;
  double p[3][3];
  CellBox box;
  const bool ok = load_triangle(v, V, tri, t, p) && cell_box(c, p, &box);
  if (!ok) atomicOr(flag, 1);
  counts[t] = ok ? box_cells(box) : 0;
}

__global__ void __launch_bounds__(kMeshThreads) meshdist_emit_kernel(const double* v, int64_t V, const int32_t* tri, int64_t T, Cells c,
                                                                    const int64_t* offsets, int64_t n_pairs, int64_t* words, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (t >= T) return;
  double p[3][3];
  CellBox box;
  if (!(load_triangle(v, V, tri, t, p) && cell_box(c, p, &box))) { atomicOr(flag, 1); return; }
  int64_t at = offsets[t];
  if (at < 0 || at > n_pairs || box_cells(box) > n_pairs - at) { atomicOr(flag, 1); return; }
  for (int x = box.lo[0]; x <= box.hi[0]; ++x)
    for (int y = box.lo[1]; y <= box.hi[1]; ++y)
      for (int z = box.lo[2]; z <= box.hi[2]; ++z) words[at++] = cell_of(c.res, x, y, z) << kMeshTriBits | t;
}

// a word that names no cell of the grid or no triangle becomes the key -1, which the cell kernels pass over
__global__ void __launch_bounds__(kMeshThreads) meshdist_unpack_kernel(const int64_t* words, int64_t n, int64_t cells, int64_t T, int64_t* keys,
                                                                      int32_t* tris, int* flag) {
  const int64_t j = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t w = words[j];
  const int64_t key = w >> kMeshTriBits, t = w & (((int64_t)1 << kMeshTriBits) - 1);
  const bool ok = w >= 0 && key < cells && t < T;
  if (!ok) atomicOr(flag, 1);
  keys[j] = ok ? key : -1;
  tris[j] = ok ? (int32_t)t : -1;
}

__global__ void __launch_bounds__(kMeshThreads) meshdist_pack_kernel(const double* v, int64_t V, const int32_t* tri, int64_t T, double* packed,
                                                                    int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (t >= T) return;
  double p[3][3];
  if (!load_triangle(v, V, tri, t, p)) atomicOr(flag, 1);
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) packed[t * 9 + j * 3 + k] = p[j][k];
}

struct MeshCells {
  Target cells;              // q unused: the runs are pairs
  const int32_t* tris;       // [n_pairs], the triangle of every pair, in cell order
  int64_t n_pairs;
  const double* packed;      // [T,9]
  int64_t T;
};

// One thread per point.  The shells are those of nearest_offgrid (offgrid.hip): clipped to the grid, beginning with the first
// that touches it, ending with the last.  After shell w every triangle not met lies farther than w h, so the walk ends once
// min(best, gate2) < kShellKeep (w h)^2 (point_triangle.h argues the factor): nothing unmet can lower best, tie with it, or
// come within the gate.
__global__ void __launch_bounds__(kMeshThreads) meshdist_query_kernel(const double* points, int64_t N, const int32_t* order, MeshCells m,
                                                                     double gate2, double* best_out, int32_t* nearest_out,
                                                                     int32_t* evaluated_out, int* flag) {
  const int64_t s = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (s >= N) return;
  const int64_t i = order ? (int64_t)order[s] : s;
  if (i < 0 || i >= N) { atomicOr(flag, 1); return; }
  const double p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
  const Cells& c = m.cells.c;
  const int origin[3] = {c.ox, c.oy, c.oz};
  int cell[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor(p[k] / c.h) - (double)origin[k];
    ok = ok && fabs(p[k]) < kMeshLimit && f > -kCellLimit && f < kCellLimit;
    cell[k] = ok ? (int)f : 0;
  }
  double best = INFINITY;
  int32_t nearest = -1, evaluated = 0;
  if (ok) {
    const int last = c.res - 1;
    int w = 0, w_end = 0;
    for (int a = 0; a < 3; ++a) {
      w = max(w, max(-cell[a], cell[a] - last));
      w_end = max(w_end, max(abs(cell[a]), abs(cell[a] - last)));
    }
    auto visit = [&](int x, int y, int z) {
      for_each_in_cell(m.cells, x, y, z, [&](int32_t j) {
        if (j < 0 || j >= m.n_pairs) return;
        const int32_t t = m.tris[j];
        if (t < 0 || t >= m.T) return;
        const double* q = m.packed + (int64_t)t * 9;
        const double a[3] = {q[0], q[1], q[2]}, b[3] = {q[3], q[4], q[5]}, cc[3] = {q[6], q[7], q[8]};
        const double d = point_triangle_d2(p, a, b, cc);
        ++evaluated;
        if (d < best || (d == best && t < nearest)) { best = d; nearest = t; }
      });
    };
    for (;; ++w) {
      for (int x = max(cell[0] - w, 0); x <= min(cell[0] + w, last); ++x)
        for (int y = max(cell[1] - w, 0); y <= min(cell[1] + w, last); ++y) {
          const int z0 = cell[2] - w, z1 = cell[2] + w;
          if (abs(x - cell[0]) == w || abs(y - cell[1]) == w) {           // a side of the shell (all of shell 0): the whole column
            for (int z = max(z0, 0); z <= min(z1, last); ++z) visit(x, y, z);
          } else {                                                        // its two ends
            if ((unsigned)z0 <= (unsigned)last) visit(x, y, z0);
            if ((unsigned)z1 <= (unsigned)last) visit(x, y, z1);
          }
        }
      const double reach = (double)w * c.h;
      if (fmin(best, gate2) < kShellKeep * (reach * reach) || w >= w_end) break;
    }
    if (best > gate2) { best = INFINITY; nearest = -1; }                  // far; best == gate2 is not
  } else {
    atomicOr(flag, 1);
    best = NAN;
  }
  best_out[i] = best;
  nearest_out[i] = nearest;
  evaluated_out[i] = evaluated;
}

// partial[k * kMeshBlocks + b], k = sum of best, max of best over the points that are not far; counts[k * kMeshBlocks + b], k =
// the far points, the candidates evaluated.  The caller's order: thread i takes i, i + threads, ...
__global__ void __launch_bounds__(kMeshThreads) meshdist_reduce_kernel(const double* best, const int32_t* evaluated, int64_t N, double* partial,
                                                                      long long* counts) {
  __shared__ double sh[2][kMeshThreads];
  __shared__ long long shc[2][kMeshThreads];
  double sum = 0.0, top = 0.0;
  long long far = 0, cand = 0;
  for (int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kMeshThreads) {
    const double d = best[i];
    if (d == INFINITY) {
      ++far;
    } else {
      sum += d;
      top = fmax(top, d);
    }
    cand += evaluated[i];
  }
  sh[0][threadIdx.x] = sum;
  sh[1][threadIdx.x] = top;
  shc[0][threadIdx.x] = far;
  shc[1][threadIdx.x] = cand;
  __syncthreads();
  for (int o = kMeshThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + o]);
      shc[0][threadIdx.x] += shc[0][threadIdx.x + o];
      shc[1][threadIdx.x] += shc[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) {
    partial[threadIdx.x * kMeshBlocks + blockIdx.x] = sh[threadIdx.x][0];
    counts[threadIdx.x * kMeshBlocks + blockIdx.x] = shc[threadIdx.x][0];
  }
}

// out4 = mean and maximum of best over the points that are not far (NaN where every point is far), the far points, the
// candidates evaluated; a raised flag makes all four NaN
__global__ void meshdist_final_kernel(const double* partial, const long long* counts, int nb, int64_t N, const int* flag, double* out4) {
  if (threadIdx.x != 0) return;
  double sum = 0.0, top = 0.0;
  long long far = 0, cand = 0;
  for (int b = 0; b < nb; ++b) {
    sum += partial[b];
    top = fmax(top, partial[kMeshBlocks + b]);
    far += counts[b];
    cand += counts[kMeshBlocks + b];
  }
  const long long counted = (long long)N - far;
  const bool bad = *flag != 0;
  out4[0] = bad || counted <= 0 ? (double)NAN : sum / (double)counted;
  out4[1] = bad || counted <= 0 ? (double)NAN : top;
  out4[2] = bad ? (double)NAN : (double)far;
  out4[3] = bad ? (double)NAN : (double)cand;
}

__global__ void __launch_bounds__(kMeshThreads) meshdist_flag_fill_kernel(const int* flag, int64_t N, double* best, int32_t* nearest) {
  const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  if (i >= N || !*flag) return;
  best[i] = NAN;
  nearest[i] = -1;
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool mesh_sizes_ok(int64_t V, int64_t T) { return V >= 1 && V <= 0x7FFFFFFF && T >= 1 && T <= 0x7FFFFFFF / 3; }

bool mesh_grid_ok(double h, int ox, int oy, int oz, int res) {
  return edge_ok(h) && res >= 1 && res <= kOffgridMaxRes && std::abs((double)ox) < kCellLimit && std::abs((double)oy) < kCellLimit &&
         std::abs((double)oz) < kCellLimit;
}

struct MeshBuffers {
  CellBuffers cells;         // rank structure, keys [n_pairs], start [n_pairs + 1]
  int32_t* tris;             // [n_pairs]
  int32_t* evaluated;        // [n_points]
  double* partial;           // [2, kMeshBlocks]
  long long* counts;         // [2, kMeshBlocks]
  size_t bytes;
};

MeshBuffers mesh_layout(int res, int64_t n_pairs, int64_t n_points, void* workspace) {
  MeshBuffers b;
  b.cells = cell_buffer_layout(res, n_pairs, workspace);
  Carver& c = b.cells.rest;
  b.tris = c.take<int32_t>((size_t)n_pairs);
  b.evaluated = c.take<int32_t>((size_t)n_points);
  b.partial = c.take<double>(2 * kMeshBlocks);
  b.counts = c.take<long long>(2 * kMeshBlocks);
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_meshdist_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double h, int ox, int oy,
                        int oz, int res, int64_t* counts, int32_t* flag, pcgc_stream_t stream) {
  PCGC_REQUIRE(vertices && triangles && counts && flag && mesh_sizes_ok(n_vertices, n_triangles) && mesh_grid_ok(h, ox, oy, oz, res),
               "pcgc_meshdist_count: bad arguments (cell edge a power of two >= 1, res 1..%d)", kOffgridMaxRes);
  hipLaunchKernelGGL(meshdist_count_kernel, dim3(mesh_blocks(n_triangles)), dim3(kMeshThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     triangles, n_triangles, Cells{h, ox, oy, oz, res}, counts, flag);
  return launch_ok("meshdist_count_kernel");
}

int pcgc_meshdist_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double h, int ox, int oy,
                       int oz, int res, const int64_t* offsets, int64_t n_pairs, int64_t* words, int32_t* flag, pcgc_stream_t stream) {
  PCGC_REQUIRE(vertices && triangles && offsets && words && flag && mesh_sizes_ok(n_vertices, n_triangles) &&
                   mesh_grid_ok(h, ox, oy, oz, res) && n_pairs >= 1 && n_pairs < 0x7FFFFFFF,
               "pcgc_meshdist_emit: bad arguments (cell edge a power of two >= 1, res 1..%d, pairs below 2^31)", kOffgridMaxRes);
  hipLaunchKernelGGL(meshdist_emit_kernel, dim3(mesh_blocks(n_triangles)), dim3(kMeshThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     triangles, n_triangles, Cells{h, ox, oy, oz, res}, offsets, n_pairs, words, flag);
  return launch_ok("meshdist_emit_kernel");
}

size_t pcgc_meshdist_workspace_bytes(int res, int64_t n_pairs, int64_t n_points) {
  if (res < 1 || res > kOffgridMaxRes || n_pairs < 1 || n_pairs >= 0x7FFFFFFF || n_points < 1 || n_points > 0x7FFFFFFF) return 0;
  return mesh_layout(res, n_pairs, n_points, nullptr).bytes;
}

int pcgc_meshdist_prepare(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const int64_t* words,
                          int64_t n_pairs, int res, int64_t n_points, double* packed, int32_t* flag, void* workspace, size_t workspace_bytes,
                          pcgc_stream_t stream) {
  PCGC_REQUIRE(vertices && triangles && words && packed && flag && workspace && mesh_sizes_ok(n_vertices, n_triangles),
               "pcgc_meshdist_prepare: bad arguments");
  const size_t need = pcgc_meshdist_workspace_bytes(res, n_pairs, n_points);
  PCGC_REQUIRE(need && workspace_bytes >= need, "pcgc_meshdist_prepare: bad sizes or workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const MeshBuffers b = mesh_layout(res, n_pairs, n_points, workspace);
  hipLaunchKernelGGL(meshdist_pack_kernel, dim3(mesh_blocks(n_triangles)), dim3(kMeshThreads), 0, s, vertices, n_vertices, triangles,
                     n_triangles, packed, flag);
  hipLaunchKernelGGL(meshdist_unpack_kernel, dim3(mesh_blocks(n_pairs)), dim3(kMeshThreads), 0, s, words, n_pairs, (int64_t)res * res * res,
                     n_triangles, b.cells.keys, b.tris, flag);
  const int rc = build_rank(b.cells.r, res, nullptr, b.cells.keys, n_pairs, s);
  if (rc) return rc;
  // a run of key -1 (a refused word) writes no start; every occupied cell has a first pair, so every entry the walk reads is written
  hipLaunchKernelGGL(offgrid_starts_kernel, dim3(mesh_blocks(n_pairs)), dim3(256), 0, s, b.cells.keys, n_pairs, b.cells.r.bits, b.cells.r.rank,
                     b.cells.r.n_set, b.cells.start, flag);
  return launch_ok("mesh distance cell kernels");
}

int pcgc_meshdist_query(const double* points, int64_t n_points, const int32_t* order, const double* packed, int64_t n_triangles,
                        int64_t n_pairs, double h, int ox, int oy, int oz, int res, double max_dist, double* out4, double* best,
                        int32_t* nearest, int32_t* flag, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && packed && out4 && best && nearest && flag && workspace && n_triangles >= 1 && n_triangles <= 0x7FFFFFFF / 3 &&
                   mesh_grid_ok(h, ox, oy, oz, res), "pcgc_meshdist_query: bad arguments");
  PCGC_REQUIRE(max_dist > 0.0, "pcgc_meshdist_query: max_dist must be positive, or +infinity for no gate (got %g)", max_dist);
  const size_t need = pcgc_meshdist_workspace_bytes(res, n_pairs, n_points);
  PCGC_REQUIRE(need && workspace_bytes >= need, "pcgc_meshdist_query: bad sizes or workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const MeshBuffers b = mesh_layout(res, n_pairs, n_points, workspace);              // as pcgc_meshdist_prepare left it
  const MeshCells m{Target{Cells{h, ox, oy, oz, res}, b.cells.r.bits, b.cells.r.rank, b.cells.start, nullptr}, b.tris, n_pairs, packed,
                    n_triangles};
  PCGC_CHECK_HIP(hipMemsetAsync(b.evaluated, 0, (size_t)n_points * sizeof(int32_t), s));
  hipLaunchKernelGGL(meshdist_query_kernel, dim3(mesh_blocks(n_points)), dim3(kMeshThreads), 0, s, points, n_points, order, m,
                     max_dist * max_dist, best, nearest, b.evaluated, flag);
  hipLaunchKernelGGL(meshdist_flag_fill_kernel, dim3(mesh_blocks(n_points)), dim3(kMeshThreads), 0, s, flag, n_points, best, nearest);
  const int blocks = (int)std::min<int64_t>((n_points + kMeshThreads - 1) / kMeshThreads, kMeshBlocks);
  hipLaunchKernelGGL(meshdist_reduce_kernel, dim3(blocks), dim3(kMeshThreads), 0, s, best, b.evaluated, n_points, b.partial, b.counts);
  hipLaunchKernelGGL(meshdist_final_kernel, dim3(1), dim3(64), 0, s, b.partial, b.counts, blocks, n_points, flag, out4);
  return launch_ok("mesh distance query kernels");
}

}  // extern "C"
