// D1 / D2 between clouds that are NOT on the integer grid (gfx950): pc_error's figures for a reconstruction scaled back by
// 1 / scale, or for any two float32 clouds.  DESIGN.md "D1 / D2 off the grid" states the rule; tests/_offgrid_ref.py
// restates it in numpy by brute force.
//
// The target cloud Q is bucketed into cubic cells of edge h (a power of two): cell = floor(q / h) - origin per axis, inside
// a grid of res^3 cells.  Coordinates are never shifted or rescaled: every distance is float64 arithmetic on the float32
// coordinates as they came, d2 = (dx*dx + dy*dy) + dz*dz with dx = double(p.x) - double(q.x) (the file is built with
// -ffp-contract=off).  The cells are the occupancy bit set and rank table of voxel_grid.h; Q comes sorted by cell key, so
// start[rank of a cell] .. start[rank + 1] are the points of that cell, any number of them.  The cells, the kernels that
// build them, the walk over a window of them and dist2 are in offgrid_cells.h, which global.hip, smooth.hip and color_icp.hip share.
//
// One thread per source point p, two passes:
//   1. Chebyshev shells of cells around p's cell, clipped to the grid, keeping the minimal d2.  A point in an unvisited
//      shell w' > w is farther than w h, so the walk ends after shell w once best + 1e-8 <= (w h)^2 — or when the grid is
//      exhausted, which bounds the walk for a p outside Q's box.
//   2. every point of the cube of those shells with |d2 - best| < 1e-8: pc_error's tie rule, no cap on their number.
// Normal sums are 2^40 fixed-point int64 atomics (exact, order-free); the mse sums are float64 in a fixed order (per
// thread, then a tree per workgroup, then the workgroups in index order).
//
// Input that breaks the contract (Q not sorted by cell or outside the grid, a coordinate whose cell no int holds, a NaN)
// is met with no index out of bounds: it raises a flag in the workspace and the outputs come back as NaN.
#include <algorithm>
#include <cmath>
#include "common.h"
#include "offgrid_cells.h"     // Cells, Target, the cell kernels, dist2, window_of, for_each_in_window / _cell, grid_ok, build_cells

namespace pcgc {
namespace {

constexpr int kOffgridBlocks = 1024;
constexpr double kTieEps = 1e-8;                    // on squared distances, absolute
constexpr double kNormalFix = 1099511627776.0;      // 2^40 fixed point for the normal sums

// ---------------------------------------------------------------------------------------------------------------- search
// Pass 1: the minimal d2 from p (in cell `cell`, which may lie outside the grid) to Q, and in *shell the last shell walked.
// Shells before the first one that touches the grid hold nothing and are skipped; the last one that touches it ends the walk.
__device__ __forceinline__ double nearest_offgrid(const Target& t, const int cell[3], double px, double py, double pz, int* shell) {
  const int last = t.c.res - 1;
  int w = 0, w_end = 0;
  for (int a = 0; a < 3; ++a) {
    w = max(w, max(-cell[a], cell[a] - last));
    w_end = max(w_end, max(abs(cell[a]), abs(cell[a] - last)));
  }
  double best = INFINITY;
  auto visit = [&](int x, int y, int z) {
    for_each_in_cell(t, x, y, z, [&](int32_t j) { best = fmin(best, dist2(t.q + (int64_t)j * 3, px, py, pz)); });
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
    const double reach = (double)w * t.c.h;
    if (best + kTieEps <= reach * reach || w >= w_end) break;
  }
  *shell = w;
  return best;
}

// Pass 2: f(j, dx, dy, dz) with d = p - q_j for every point of Q within 1e-8 of `best`, cells in x, y, z order, the points
// of a cell in Q's order
template <typename F>
__device__ __forceinline__ void for_each_tied_offgrid(const Target& t, const int cell[3], double px, double py, double pz, double best,
                                                      int shell, F f) {
  for_each_in_window(t, window_of(cell, shell, t.c.res), [&](int32_t j) {
    const float* q = t.q + (int64_t)j * 3;
    if (fabs(dist2(q, px, py, pz) - best) < kTieEps) f(j, px - (double)q[0], py - (double)q[1], pz - (double)q[2]);
  });
}

// ---------------------------------------------------------------------------------------------------------------- normals
__global__ void __launch_bounds__(256) offgrid_transfer_kernel(const float* p, int64_t np, const float* normals_p, Target t,
                                                               long long* sums, int* counts, int* bad) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
    int cell[3], shell;
    if (!cell_of_point(t.c, p + i * 3, cell)) { atomicOr(bad, 1); continue; }
    const double px = p[i * 3], py = p[i * 3 + 1], pz = p[i * 3 + 2];
    const double best = nearest_offgrid(t, cell, px, py, pz, &shell);
    long long fx[3];
    for (int c = 0; c < 3; ++c) fx[c] = (long long)llrint((double)normals_p[i * 3 + c] * kNormalFix);
    for_each_tied_offgrid(t, cell, px, py, pz, best, shell, [&](int32_t j, double, double, double) {
      for (int c = 0; c < 3; ++c) atomicAdd(reinterpret_cast<unsigned long long*>(&sums[(int64_t)j * 3 + c]), (unsigned long long)fx[c]);
      atomicAdd(&counts[j], 1);
    });
  }
}

__global__ void __launch_bounds__(256) offgrid_normals_final_kernel(const long long* sums, const int* counts, int64_t nq, const int* bad,
                                                                    double* normals_q) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  const int c = counts[j];
  for (int k = 0; k < 3; ++k)
    normals_q[j * 3 + k] = *bad ? (double)NAN : (c ? (double)sums[j * 3 + k] / kNormalFix / (double)c : 0.0);
}

// ---------------------------------------------------------------------------------------------------------------- mse
// partial[k * kOffgridBlocks + b], k = sum of best, max of best, sum of plane, max of plane of workgroup b
__global__ void __launch_bounds__(256) offgrid_mse_partial_kernel(const float* p, int64_t np, Target t, const double* normals_q,
                                                                  double* partial, double* best_out, double* plane_out,
                                                                  int32_t* ties_out, int* bad) {
  __shared__ double sh[4][256];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
    int cell[3], shell, ties = 0;
    double best = NAN, plane = 0.0;
    if (cell_of_point(t.c, p + i * 3, cell)) {
      const double px = p[i * 3], py = p[i * 3 + 1], pz = p[i * 3 + 2];
      best = nearest_offgrid(t, cell, px, py, pz, &shell);
      double s = 0.0;
      for_each_tied_offgrid(t, cell, px, py, pz, best, shell, [&](int32_t j, double dx, double dy, double dz) {
        if (normals_q) {
          const double* n = normals_q + (int64_t)j * 3;
          const double d = (dx * n[0] + dy * n[1]) + dz * n[2];
          s += d * d;
        }
        ++ties;
      });
      if (ties) plane = s / (double)ties;
    } else {
      atomicOr(bad, 1);
    }
    if (best_out) { best_out[i] = best; plane_out[i] = plane; ties_out[i] = ties; }
    acc[0] += best; acc[1] = fmax(acc[1], best);
    acc[2] += plane; acc[3] = fmax(acc[3], plane);
  }
  for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + o]);
      sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
      sh[3][threadIdx.x] = fmax(sh[3][threadIdx.x], sh[3][threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) partial[threadIdx.x * kOffgridBlocks + blockIdx.x] = sh[threadIdx.x][0];
}

__global__ void offgrid_mse_final_kernel(const double* partial, int nb, int64_t np, int with_plane, const int* bad, double* out4) {
  if (threadIdx.x != 0) return;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < nb; ++i) {
    v[0] += partial[i];
    v[1] = fmax(v[1], partial[kOffgridBlocks + i]);
    v[2] += partial[2 * kOffgridBlocks + i];
    v[3] = fmax(v[3], partial[3 * kOffgridBlocks + i]);
  }
  v[0] /= (double)np;
  v[2] /= (double)np;
  for (int k = 0; k < 4; ++k) out4[k] = *bad ? (double)NAN : ((k < 2 || with_plane) ? v[k] : 0.0);
}

// ---------------------------------------------------------------------------------------------------------------- registration
// One ICP step (include/pcgc.h, pcgc_register_step and pcgc_register_color_step; tests/_register_ref.py, _color_icp_ref.py): the
// source under a trial pose, its tied nearest neighbours within the gate, and float64 sums over the pairs in a fixed order.  ONE
// kernel does the search, the gate, the ties and the reduction; WHICH sums a pair adds to is a small "terms" policy:
//   PlaneTerms  45 sums: the point-to-point moments and, with normals, the point-to-plane normal equations
//   ColorTerms  59 sums: the point-to-plane block, the count of valid pairs, the photometric block over the
//               target's intensity gradients (pcgc_color_gradient, color_icp.hip); no moments, so the sums stay in registers
// Sums 0 and 1 are the number of source points used and the sum of their best d2 in both.  The pose travels as a kernel argument.
struct Pose {
  double R[9], t[3], c[3];
};

// a block of 28: acc[0..20] += (w J_r) J_c for r <= c, acc[21..26] += (w J_r) res, acc[27] += (w res) res
__device__ __forceinline__ void add_six_terms(double* acc, const double J[6], double res, double w) {
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double wj = w * J[r];
#pragma unroll
    for (int c = r; c < 6; ++c) acc[k++] += wj * J[c];
    acc[21 + r] += wj * res;
  }
  acc[27] += (w * res) * res;
}

// the point-to-plane block of the pair (a, b) with the target's normal n
__device__ __forceinline__ void add_plane_terms(double* acc, const double a[3], const double b[3], const float* n, double w) {
  const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
  const double res = ((a[0] - b[0]) * n0 + (a[1] - b[1]) * n1) + (a[2] - b[2]) * n2;
  const double J[6] = {a[1] * n2 - a[2] * n1, a[2] * n0 - a[0] * n2, a[0] * n1 - a[1] * n0, n0, n1, n2};
  add_six_terms(acc, J, res, w);
}

// A terms policy: kSums accumulators; source(i), read once per source point that passes the gate; add(), the terms of the pair
// of that point at a = p - c with target point j at b = q_j - c, weight w; and the names its entry point reports under.
struct PlaneTerms {
  static constexpr int kSums = 45;
  static constexpr const char* kName = "pcgc_register_step";
  static constexpr const char* kKernels = "registration step kernels";
  const float* normals_q;                                    // or null: acc[17 ..] is left alone

  __device__ __forceinline__ double source(int64_t) const { return 0.0; }
  __device__ __forceinline__ void add(double* acc, double, const double a[3], const double b[3], int32_t j, double w) const {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double wa = w * a[r];
      acc[2 + r] += wa;
      acc[5 + r] += w * b[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[8 + r * 3 + c] += wa * b[c];
    }
    if (normals_q) add_plane_terms(acc + 17, a, b, normals_q + (int64_t)j * 3, w);
  }
};

constexpr double kIntensityScale = 2550000.0;                       // 255 * (2126 + 7152 + 722)

struct ColorTerms {
  static constexpr int kSums = 59;
  static constexpr int kGeo = 2, kWeight = 30, kPhoto = 31;         // where the two blocks of 28 and the weight sum start
  static constexpr const char* kName = "pcgc_register_color_step";
  static constexpr const char* kKernels = "colour registration step kernels";
  const int32_t* Yp;
  const float* normals_q;
  const int32_t* Yq;
  const double* grad_q;
  const uint8_t* valid_q;

  __device__ __forceinline__ double source(int64_t i) const { return (double)Yp[i] / kIntensityScale; }
  __device__ __forceinline__ void add(double* acc, double ip, const double a[3], const double b[3], int32_t j, double w) const {
    add_plane_terms(acc + kGeo, a, b, normals_q + (int64_t)j * 3, w);
    if (!valid_q[j]) return;
    const double* g = grad_q + (int64_t)j * 3;
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    const double rc = ((double)Yq[j] / kIntensityScale - ip) + (((a[0] - b[0]) * g0 + (a[1] - b[1]) * g1) + (a[2] - b[2]) * g2);
    const double Jc[6] = {a[1] * g2 - a[2] * g1, a[2] * g0 - a[0] * g2, a[0] * g1 - a[1] * g0, g0, g1, g2};
    acc[kWeight] += w;
    add_six_terms(acc + kPhoto, Jc, rc, w);
  }
};

// partial[k * kOffgridBlocks + b] = sum k of workgroup b.  The accumulators of a thread stay in registers; the workgroup's
// sum is a shuffle tree per wave, then the four waves in order (4 x kSums doubles of LDS, not kSums x 256).
template <typename Terms>
__global__ void __launch_bounds__(256) register_step_kernel(const float* p, int64_t np, Target t, Terms terms, Pose pose, double gate2,
                                                            double* partial, double* best_out, int32_t* ties_out, int* bad) {
  constexpr int kSums = Terms::kSums;
  __shared__ double sh[4][kSums];
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  long long n_used = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
    const double x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    float pf[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pf[r] = (float)(((pose.R[3 * r] * x + pose.R[3 * r + 1] * y) + pose.R[3 * r + 2] * z) + pose.t[r]);
    int cell[3], shell, ties = 0;
    double best = NAN;
    if (cell_of_point(t.c, pf, cell)) {
      const double px = pf[0], py = pf[1], pz = pf[2];
      best = nearest_offgrid(t, cell, px, py, pz, &shell);
      if (best <= gate2) {
        for_each_tied_offgrid(t, cell, px, py, pz, best, shell, [&](int32_t, double, double, double) { ++ties; });
        const double w = 1.0 / (double)ties;
        const double a[3] = {px - pose.c[0], py - pose.c[1], pz - pose.c[2]};
        const double from_source = terms.source(i);
        for_each_tied_offgrid(t, cell, px, py, pz, best, shell, [&](int32_t j, double, double, double) {
          const float* q = t.q + (int64_t)j * 3;
          const double b[3] = {(double)q[0] - pose.c[0], (double)q[1] - pose.c[1], (double)q[2] - pose.c[2]};
          terms.add(acc, from_source, a, b, j, w);
        });
        ++n_used;
        acc[1] += best;
      }
    } else {
      atomicOr(bad, 1);
    }
    if (best_out) { best_out[i] = best; ties_out[i] = ties; }
  }
  acc[0] = (double)n_used;                                    // below 2^31 per launch: exact, and so is every partial sum of them
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums)
    partial[threadIdx.x * kOffgridBlocks + blockIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one wave: lane k < n_sums adds sum k of the workgroups in index order; bad[0] is prepare's flag (the target), bad[1] this step's
__global__ void __launch_bounds__(64) register_final_kernel(const double* partial, int nb, int n_sums, const int* bad, double* out) {
  const int k = threadIdx.x;
  if (k >= n_sums) return;
  double v = 0.0;
  for (int i = 0; i < nb; ++i) v += partial[k * kOffgridBlocks + i];
  out[k] = (bad[0] | bad[1]) ? (double)NAN : v;
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct OffgridBuffers {
  RankBuffers r;
  int64_t* keys;             // [nq]
  int32_t* start;            // [nq + 1]
  long long* sums;           // [nq,3]
  int* counts;               // [nq]
  double* partial;           // [4, kOffgridBlocks]
  int* bad;                  // [2] the target's flag (build_target), a register step's
  double* step_partial;      // [n_sums, kOffgridBlocks]
  size_t bytes;
};

// n_sums = 0: the off-grid measures' workspace.  A register workspace is that and the steps' partial sums behind it, so what
// pcgc_register_prepare leaves is where both step kernels look for it
OffgridBuffers offgrid_layout(int res, int64_t nq, int n_sums, void* workspace) {
  OffgridBuffers b;
  b.r = rank_layout(res, workspace);
  Carver& c = b.r.rest;
  b.keys = c.take<int64_t>((size_t)nq);
  b.start = c.take<int32_t>((size_t)nq + 1);
  b.sums = c.take<long long>((size_t)nq * 3);
  b.counts = c.take<int>((size_t)nq);
  b.partial = c.take<double>(4 * kOffgridBlocks);
  b.bad = c.take<int>(2);
  b.step_partial = c.take<double>((size_t)n_sums * kOffgridBlocks);
  b.bytes = c.bytes();
  return b;
}

int build_target(const OffgridBuffers& b, const Cells& c, const float* q, int64_t nq, hipStream_t s, Target* t) {
  return build_cells(b.r, b.keys, b.start, b.bad, c, q, nq, s, t);
}

// a step of either metric against the target pcgc_register_prepare left in the workspace; pointers_ok: the entry point's own
template <typename Terms>
int register_step(const Terms& terms, bool pointers_ok, const float* p, int64_t np, const float* q, int64_t nq, double h, int ox, int oy,
                  int oz, int res, const double* R9, const double* t3, const double* c3, double max_dist, double* out, double* best,
                  int32_t* n_ties, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(pointers_ok && p && q && R9 && t3 && c3 && out && workspace && grid_ok(h, ox, oy, oz, res, np, nq) &&
               (best == nullptr) == (n_ties == nullptr), "%s: bad arguments", Terms::kName);
  PCGC_REQUIRE(std::isfinite(max_dist) && max_dist > 0.0, "%s: max_dist must be finite and positive (got %g)", Terms::kName, max_dist);
  Pose pose;
  for (int k = 0; k < 9; ++k) pose.R[k] = R9[k];
  for (int k = 0; k < 3; ++k) { pose.t[k] = t3[k]; pose.c[k] = c3[k]; }
  bool finite = true;
  for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(pose.R[k]);
  for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(pose.t[k]) && std::isfinite(pose.c[k]);
  PCGC_REQUIRE(finite, "%s: the pose and the centre must be finite", Terms::kName);
  const OffgridBuffers b = offgrid_layout(res, nq, Terms::kSums, workspace);     // as pcgc_register_prepare left it
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "%s: workspace too small", Terms::kName);
  hipStream_t s = (hipStream_t)stream;
  const Target t{Cells{h, ox, oy, oz, res}, b.r.bits, b.r.rank, b.start, q};
  PCGC_CHECK_HIP(hipMemsetAsync(b.bad + 1, 0, sizeof(int), s));
  const int blocks = (int)std::min<int64_t>((np + 255) / 256, kOffgridBlocks);
  hipLaunchKernelGGL(register_step_kernel<Terms>, dim3(blocks), dim3(256), 0, s, p, np, t, terms, pose, max_dist * max_dist, b.step_partial,
                     best, n_ties, b.bad + 1);
  hipLaunchKernelGGL(register_final_kernel, dim3(1), dim3(64), 0, s, b.step_partial, blocks, Terms::kSums, b.bad, out);
  return launch_ok(Terms::kKernels);
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_offgrid_workspace_bytes(int res, int64_t nq) { return cloud_sizes_ok(res, nq) ? offgrid_layout(res, nq, 0, nullptr).bytes : 0; }

int pcgc_offgrid_transfer_normals(const float* p, int64_t np, const float* normals_p, const float* q, int64_t nq, double h, int ox,
                                  int oy, int oz, int res, double* normals_q, void* workspace, size_t workspace_bytes,
                                  pcgc_stream_t stream) {
  PCGC_REQUIRE(p && normals_p && q && normals_q && workspace && grid_ok(h, ox, oy, oz, res, np, nq),
               "pcgc_offgrid_transfer_normals: bad arguments");
  const OffgridBuffers b = offgrid_layout(res, nq, 0, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_offgrid_transfer_normals: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_target(b, Cells{h, ox, oy, oz, res}, q, nq, s, &t);
  if (rc) return rc;
  PCGC_CHECK_HIP(hipMemsetAsync(b.sums, 0, (size_t)nq * 3 * sizeof(long long), s));
  PCGC_CHECK_HIP(hipMemsetAsync(b.counts, 0, (size_t)nq * sizeof(int), s));
  const int blocks = (int)std::min<int64_t>((np + 255) / 256, 4096);
  hipLaunchKernelGGL(offgrid_transfer_kernel, dim3(blocks), dim3(256), 0, s, p, np, normals_p, t, b.sums, b.counts, b.bad);
  hipLaunchKernelGGL(offgrid_normals_final_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, b.sums, b.counts, nq, b.bad,
                     normals_q);
  return launch_ok("off-grid normal transfer kernels");
}

int pcgc_offgrid_mse(const float* p, int64_t np, const float* q, int64_t nq, const double* normals_q, double h, int ox, int oy, int oz,
                     int res, double* out4, double* best, double* plane, int32_t* n_ties, void* workspace, size_t workspace_bytes,
                     pcgc_stream_t stream) {
  PCGC_REQUIRE(p && q && out4 && workspace && grid_ok(h, ox, oy, oz, res, np, nq) && (best == nullptr) == (plane == nullptr) &&
               (best == nullptr) == (n_ties == nullptr), "pcgc_offgrid_mse: bad arguments");
  const OffgridBuffers b = offgrid_layout(res, nq, 0, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_offgrid_mse: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_target(b, Cells{h, ox, oy, oz, res}, q, nq, s, &t);
  if (rc) return rc;
  const int blocks = (int)std::min<int64_t>((np + 255) / 256, kOffgridBlocks);
  hipLaunchKernelGGL(offgrid_mse_partial_kernel, dim3(blocks), dim3(256), 0, s, p, np, t, normals_q, b.partial, best, plane, n_ties,
                     b.bad);
  hipLaunchKernelGGL(offgrid_mse_final_kernel, dim3(1), dim3(64), 0, s, b.partial, blocks, np, normals_q ? 1 : 0, b.bad, out4);
  return launch_ok("off-grid mse kernels");
}

size_t pcgc_register_workspace_bytes(int res, int64_t nq) {
  return cloud_sizes_ok(res, nq) ? offgrid_layout(res, nq, PlaneTerms::kSums, nullptr).bytes : 0;
}

// pcgc_register_prepare fills the colour step's workspace as it fills the plain step's
size_t pcgc_register_color_workspace_bytes(int res, int64_t nq) {
  return cloud_sizes_ok(res, nq) ? offgrid_layout(res, nq, ColorTerms::kSums, nullptr).bytes : 0;
}

int pcgc_register_prepare(const float* q, int64_t nq, double h, int ox, int oy, int oz, int res, void* workspace,
                          size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(q && workspace && grid_ok(h, ox, oy, oz, res, 1, nq), "pcgc_register_prepare: bad arguments");
  const OffgridBuffers b = offgrid_layout(res, nq, PlaneTerms::kSums, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_register_prepare: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_target(b, Cells{h, ox, oy, oz, res}, q, nq, s, &t);
  if (rc) return rc;
  return launch_ok("registration target kernels");
}

int pcgc_register_step(const float* p, int64_t np, const float* q, int64_t nq, const float* normals_q, double h, int ox, int oy, int oz,
                       int res, const double* R9, const double* t3, const double* c3, double max_dist, double* out45, double* best,
                       int32_t* n_ties, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  return register_step(PlaneTerms{normals_q}, true, p, np, q, nq, h, ox, oy, oz, res, R9, t3, c3, max_dist, out45, best, n_ties, workspace,
                       workspace_bytes, stream);
}

int pcgc_register_color_step(const float* p, const int32_t* Yp, int64_t np, const float* q, const float* normals_q, const int32_t* Yq,
                             const double* grad_q, const uint8_t* valid_q, int64_t nq, double h, int ox, int oy, int oz, int res,
                             const double* R9, const double* t3, const double* c3, double max_dist, double* out59, double* best,
                             int32_t* n_ties, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  return register_step(ColorTerms{Yp, normals_q, Yq, grad_q, valid_q}, Yp && normals_q && Yq && grad_q && valid_q, p, np, q, nq, h, ox, oy,
                       oz, res, R9, t3, c3, max_dist, out59, best, n_ties, workspace, workspace_bytes, stream);
}

}  // extern "C"
