// Smoothing of a float32 scan before it is voxelised (gfx950): every point is projected onto the plane fitted to the points
// within `radius` of it, which thins the shell of several voxels that range noise and residual pose error leave around a
// surface.  include/pcgc.h (pcgc_smooth_*) and DESIGN.md §7j state the rule; tests/_smooth_ref.py restates it in numpy;
// pcgcv1_amd/smooth.py chains the passes.
//
// The neighbourhood's moments are exact integers (offsets in 2^-16 of a grid unit, summed in int64), so they do not depend on
// the order the neighbours are met in; everything behind them is IEEE float64, one operation per step in the order written
// (-ffp-contract=off), and the eigenvector comes from the Jacobi loop the normal estimation uses (jacobi3.h).  The device and
// numpy therefore agree bit for bit.
//
// One thread per point, the points in cell order (offgrid_cells.h): the lanes of a wave lie in the same or neighbouring
// cells, so they walk the same 27 cell ranges (for_each_in_window) and their loads of the neighbours coincide.  The ten sums
// and the count live in registers; there are no atomics on data and no scratch (DESIGN.md §7j quotes the register counts).
// Input that breaks the contract (points not sorted by cell or outside the grid, a coordinate that is not finite) is met
// with no index out of bounds: it raises the flag in the workspace, and `moved` says so.
#include <cmath>
#include "common.h"
#include "jacobi3.h"
#include "offgrid_cells.h"

namespace pcgc {
namespace {

constexpr double kSmoothMaxRadius = 16.0;           // |offset| <= 2^20, a product below 2^41
constexpr int kSmoothMaxK = 1 << 22;                // ... so 2^22 terms stay inside int64
constexpr double kSmoothScale = 65536.0;

__global__ void __launch_bounds__(256) smooth_step_kernel(Target t, int64_t n, double r2, int kmin, float* out, uint8_t* moved,
                                                          int32_t* Kout, int64_t* Sout, int64_t* Qout, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* g = t.q + i * 3;
  const double px = g[0], py = g[1], pz = g[2];
  int K = 0;
  int64_t s0 = 0, s1 = 0, s2 = 0, q00 = 0, q01 = 0, q02 = 0, q11 = 0, q12 = 0, q22 = 0;
  bool dense = false;
  int cell[3];
  if (cell_of_point(t.c, g, cell)) {
    for_each_in_window(t, window_of(cell, 1, t.c.res), [&](int32_t j) {
      const float* q = t.q + (int64_t)j * 3;
      if (!(dist2(q, px, py, pz) <= r2)) return;           // false for a NaN
      if (K == kSmoothMaxK) {
        dense = true;
        return;
      }
      const int64_t a = llrint(((double)q[0] - px) * kSmoothScale);
      const int64_t b = llrint(((double)q[1] - py) * kSmoothScale);
      const int64_t c = llrint(((double)q[2] - pz) * kSmoothScale);
      ++K;
      s0 += a; s1 += b; s2 += c;
      q00 += a * a; q01 += a * b; q02 += a * c; q11 += b * b; q12 += b * c; q22 += c * c;
    });
  } else {
    atomicOr(bad, kFlagInput);
  }
  if (dense) atomicOr(bad, kFlagDense);
  if (Kout) {
    Kout[i] = K;
    Sout[i * 3] = s0; Sout[i * 3 + 1] = s1; Sout[i * 3 + 2] = s2;
    Qout[i * 6] = q00; Qout[i * 6 + 1] = q01; Qout[i * 6 + 2] = q02; Qout[i * 6 + 3] = q11; Qout[i * 6 + 4] = q12; Qout[i * 6 + 5] = q22;
  }
  const unsigned* gbits = reinterpret_cast<const unsigned*>(g);
  unsigned* obits = reinterpret_cast<unsigned*>(out + i * 3);
  if (K < kmin) {                                   // not moved: the bits of the input
    obits[0] = gbits[0]; obits[1] = gbits[1]; obits[2] = gbits[2];
    moved[i] = 0;
    return;
  }
  const double dk = (double)K;
  const double m0 = (double)s0 / dk, m1 = (double)s1 / dk, m2 = (double)s2 / dk;
  double a[3][3], v[3][3];
  a[0][0] = (double)q00 / dk - m0 * m0;
  a[0][1] = a[1][0] = (double)q01 / dk - m0 * m1;
  a[0][2] = a[2][0] = (double)q02 / dk - m0 * m2;
  a[1][1] = (double)q11 / dk - m1 * m1;
  a[1][2] = a[2][1] = (double)q12 / dk - m1 * m2;
  a[2][2] = (double)q22 / dk - m2 * m2;
  jacobi3(a, v);
  const int jx = a[1][1] < a[0][0] ? (a[2][2] < a[1][1] ? 2 : 1) : (a[2][2] < a[0][0] ? 2 : 0);
  double nrm[3];
  for (int k = 0; k < 3; ++k) nrm[k] = jx == 0 ? v[k][0] : jx == 1 ? v[k][1] : v[k][2];
  const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
  for (int k = 0; k < 3; ++k) nrm[k] /= len;
  // no sign rule: the move is (m . n) n, and (-t)(-n) has the bits of t n
  const double tt = (m0 * nrm[0] + m1 * nrm[1]) + m2 * nrm[2];
  const double d = tt / kSmoothScale;
  out[i * 3] = (float)(px + d * nrm[0]);
  out[i * 3 + 1] = (float)(py + d * nrm[1]);
  out[i * 3 + 2] = (float)(pz + d * nrm[2]);
  moved[i] = 1;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_smooth_workspace_bytes(int res, int64_t n) { return cloud_sizes_ok(res, n) ? cell_buffer_layout(res, n, nullptr).bytes : 0; }

int pcgc_smooth_step(const float* points, int64_t n, double h, int ox, int oy, int oz, int res, double radius, int kmin, float* out,
                     uint8_t* moved, int32_t* K, int64_t* S, int64_t* Q, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && out && moved && workspace && out != points && cloud_sizes_ok(res, n) && grid_ok(h, ox, oy, oz, res, n, n),
               "pcgc_smooth_step: bad arguments");
  PCGC_REQUIRE((K != nullptr) == (S != nullptr) && (K != nullptr) == (Q != nullptr), "pcgc_smooth_step: K, S and Q come together or not at all");
  PCGC_REQUIRE(std::isfinite(radius) && radius > 0.0 && radius <= kSmoothMaxRadius && radius <= h,
               "pcgc_smooth_step: radius %g must be positive, at most %g and at most the cell edge %g", radius, kSmoothMaxRadius, h);
  PCGC_REQUIRE(kmin >= 3 && kmin <= kSmoothMaxK, "pcgc_smooth_step: kmin %d outside 3..%d", kmin, kSmoothMaxK);
  const CellBuffers b = cell_buffer_layout(res, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_smooth_step: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_cells(b.r, b.keys, b.start, b.bad, Cells{h, ox, oy, oz, res}, points, n, s, &t);
  if (rc) return rc;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(smooth_step_kernel, dim3(grid), dim3(256), 0, s, t, n, radius * radius, kmin, out, moved, K, S, Q, b.bad);
  hipLaunchKernelGGL(flag_marks_kernel, dim3(grid), dim3(256), 0, s, b.bad, n, moved);
  return launch_ok("smooth kernels");
}

}  // extern "C"
