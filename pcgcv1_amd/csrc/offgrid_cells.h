// The cells a float32 cloud is searched in, and the one walk over them, shared by the off-grid D1 / D2 and registration
// kernels (offgrid.hip), the descriptor kernels of the global alignment (global.hip), the smoothing (smooth.hip) and the
// colour gradient (color_icp.hip).  The cloud Q is bucketed into cubic cells of edge h (a power of
// two): cell = floor(q / h) - origin per axis, inside a grid of res^3 cells.  Coordinates are never shifted or rescaled: every
// distance is float64 arithmetic on the float32 coordinates as they came, d2 = (dx*dx + dy*dy) + dz*dz with dx = double(p.x)
// - double(q.x) (the including files are built with -ffp-contract=off).  The cells are the occupancy bit set and rank table
// of voxel_grid.h; Q comes sorted by cell key, so start[rank of a cell] .. start[rank + 1] are the points of that cell, any
// number of them.  Everything here has internal linkage: the objects link into one library.
#pragma once
#include <cmath>
#include "common.h"
#include "voxel_grid.h"

namespace pcgc {
namespace {

constexpr int kOffgridMaxRes = 1024;
constexpr double kCellLimit = 536870912.0;          // 2^29: |cell - origin| and |origin| stay below it, so cell +- shell fits an int
constexpr double kMinEdge = 1.0, kMaxEdge = 1048576.0;                  // 1 .. 2^20

struct Cells {
  double h;
  int ox, oy, oz;            // the cell of the grid's corner
  int res;
};

struct Target {
  Cells c;
  const unsigned* bits;
  const unsigned* rank;
  const int32_t* start;      // [occupied cells + 1]: first point of each occupied cell in key order, then nq
  const float* q;            // [nq,3], sorted by cell key
};

// cell coordinate (relative to the grid's corner) of a coordinate; false when no int below 2^29 holds it, or for a NaN
__device__ __forceinline__ bool cell_coord(float v, double h, int origin, int* c) {
  const double f = floor((double)v / h) - (double)origin;
  if (!(f > -kCellLimit && f < kCellLimit)) return false;
  *c = (int)f;
  return true;
}

__device__ __forceinline__ bool cell_of_point(const Cells& c, const float* p, int cell[3]) {
  return cell_coord(p[0], c.h, c.ox, &cell[0]) && cell_coord(p[1], c.h, c.oy, &cell[1]) && cell_coord(p[2], c.h, c.oz, &cell[2]);
}

// ---------------------------------------------------------------------------------------------------------------- the cells of Q
// linear key of every point of Q, -1 (and the flag) for one outside the grid
__global__ void __launch_bounds__(256) offgrid_keys_kernel(const float* q, int64_t nq, Cells c, int64_t* keys, int* bad) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  int cell[3];
  int64_t key = -1;
  if (cell_of_point(c, q + j * 3, cell) && in_grid(c.res, cell[0], cell[1], cell[2])) key = cell_of(c.res, cell[0], cell[1], cell[2]);
  if (key < 0) atomicOr(bad, 1);
  keys[j] = key;
}

// start[r] = the first point of the r-th occupied cell, start[occupied cells] = nq.  Every occupied cell has a first point,
// so every entry is written, with an index within [0, nq], whatever the order of Q; keys that descend raise the flag.
__global__ void __launch_bounds__(256) offgrid_starts_kernel(const int64_t* keys, int64_t nq, const unsigned* bits, const unsigned* rank,
                                                             const int64_t* n_set, int32_t* start, int* bad) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  if (j == 0) start[*n_set] = (int32_t)nq;                  // n_set <= nq: the table has nq + 1 entries
  const int64_t key = keys[j], prev = j ? keys[j - 1] : -1;
  if (key < 0) return;
  if (prev > key) atomicOr(bad, 1);
  if (prev != key) start[rank_of(bits, rank, key)] = (int32_t)j;
}

// ---------------------------------------------------------------------------------------------------------------- search
__device__ __forceinline__ double dist2(const float* q, double px, double py, double pz) {
  const double dx = px - (double)q[0], dy = py - (double)q[1], dz = pz - (double)q[2];
  return (dx * dx + dy * dy) + dz * dz;
}

struct Window {
  int x0, x1, y0, y1, z0, z1;
};

// the cells within w of `cell`, clipped to the grid (empty when the cell lies further outside than w)
__device__ __forceinline__ Window window_of(const int cell[3], int w, int res) {
  return Window{max(cell[0] - w, 0), min(cell[0] + w, res - 1), max(cell[1] - w, 0), min(cell[1] + w, res - 1),
                max(cell[2] - w, 0), min(cell[2] + w, res - 1)};
}

// THE cell walk: calls f(first, end) with the run of points of every occupied cell of a window inside the grid, the cells in
// x, y, z order.  What a caller does with a run is its own: a thread takes every point (for_each_in_window), the lanes of a
// wave stride over it (global.hip).
template <typename F>
__device__ __forceinline__ void for_each_run(const Target& t, const Window& v, F f) {
  for (int x = v.x0; x <= v.x1; ++x)
    for (int y = v.y0; y <= v.y1; ++y)
      for (int z = v.z0; z <= v.z1; ++z) {
        if (!bit_at(t.bits, t.c.res, x, y, z)) continue;
        const int64_t r = rank_of(t.bits, t.rank, cell_of(t.c.res, x, y, z));
        f(t.start[r], t.start[r + 1]);
      }
}

// calls f(j) for every point j of the window, the points of a cell in Q's order
template <typename F>
__device__ __forceinline__ void for_each_in_window(const Target& t, const Window& v, F f) {
  for_each_run(t, v, [&](int32_t j, int32_t end) {
    for (; j < end; ++j) f(j);
  });
}

// calls f(j) for every point j of the cell (x, y, z), which lies inside the grid
template <typename F>
__device__ __forceinline__ void for_each_in_cell(const Target& t, int x, int y, int z, F f) {
  for_each_in_window(t, Window{x, x, y, y, z, z}, f);
}

// Kernels of one thread per point of the cloud itself (smooth.hip, color_icp.hip) report through a uint8 per point.  A raised
// flag overwrites all of them with one value that names the cause.
constexpr int kFlagInput = 1, kFlagDense = 2;
constexpr uint8_t kMarkBadInput = 255, kMarkTooDense = 254;

__global__ void __launch_bounds__(256) flag_marks_kernel(const int* bad, int64_t n, uint8_t* marks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int flag = *bad;
  if (i >= n || !flag) return;
  marks[i] = (flag & kFlagInput) ? kMarkBadInput : kMarkTooDense;
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool edge_ok(double h) {
  int e;
  return h >= kMinEdge && h <= kMaxEdge && std::frexp(h, &e) == 0.5;
}

bool grid_ok(double h, int ox, int oy, int oz, int res, int64_t np, int64_t nq) {
  return edge_ok(h) && res >= 1 && res <= kOffgridMaxRes && std::abs((double)ox) < kCellLimit && std::abs((double)oy) < kCellLimit &&
         std::abs((double)oz) < kCellLimit && np > 0 && nq > 0 && np <= 0x7FFFFFFF && nq < 0x7FFFFFFF;
}

// the sizes a cloud that is searched in its own cells may have (smooth.hip, color_icp.hip)
bool cloud_sizes_ok(int res, int64_t n) { return res >= 1 && res <= kOffgridMaxRes && n > 0 && n < 0x7FFFFFFF; }

// the cells of Q into r, keys [nq] and start [nq + 1]: keys, bit set, rank table, cell starts; the flag starts at zero
int build_cells(const RankBuffers& r, int64_t* keys, int32_t* start, int* bad, const Cells& c, const float* q, int64_t nq, hipStream_t s,
                Target* t) {
  const unsigned grid = (unsigned)((nq + 255) / 256);
  PCGC_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(offgrid_keys_kernel, dim3(grid), dim3(256), 0, s, q, nq, c, keys, bad);
  const int rc = build_rank(r, c.res, nullptr, keys, nq, s);
  if (rc) return rc;
  hipLaunchKernelGGL(offgrid_starts_kernel, dim3(grid), dim3(256), 0, s, keys, nq, r.bits, r.rank, r.n_set, start, bad);
  *t = Target{c, r.bits, r.rank, start, q};
  return 0;
}

// a workspace that holds the cells of a cloud of n points and nothing else: what build_cells fills (global.hip, smooth.hip)
struct CellBuffers {
  RankBuffers r;
  int64_t* keys;             // [n]
  int32_t* start;            // [n + 1]
  int* bad;
  Carver rest;               // what a larger layout puts behind the cells (meshdist.hip)
  size_t bytes;
};

CellBuffers cell_buffer_layout(int res, int64_t n, void* workspace) {
  CellBuffers b;
  b.r = rank_layout(res, workspace);
  b.rest = b.r.rest;
  Carver& c = b.rest;
  b.keys = c.take<int64_t>((size_t)n);
  b.start = c.take<int32_t>((size_t)n + 1);
  b.bad = c.take<int>(1);
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace pcgc
