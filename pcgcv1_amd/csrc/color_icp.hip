// The intensity gradient of a coloured target cloud, per point and in the point's tangent plane (gfx950): what the photometric
// term of coloured ICP (Park, Zhou, Koltun 2017) linearises a target's texture with.  include/pcgc.h (pcgc_color_gradient) and
// DESIGN.md §7k state the rule; tests/_color_icp_ref.py restates it in numpy; pcgcv1_amd/register.py calls it once per target
// and hands the result to pcgc_register_color_step (offgrid.hip).
//
// Built like smooth.hip, on the same walk (for_each_in_window), flag kernel and size check of offgrid_cells.h.  The
// least-squares sums over the ball around a point are exact integers (offsets in 2^-16 of a grid unit, intensities in
// 1 / 2 550 000, summed in int64), so they do not depend on the order the neighbours are met in; everything behind them is
// IEEE float64, one operation per step in the order written (-ffp-contract=off).  The device and numpy therefore agree bit
// for bit.
//
// One thread per point, the points in cell order (offgrid_cells.h): the lanes of a wave walk the same 27 cell ranges.  The
// nine sums and the count live in registers; there are no atomics on data, no LDS and no scratch (DESIGN.md §7k quotes the
// register counts).  Input that breaks the contract (points not sorted by cell or outside the grid, a coordinate that is not
// finite, an intensity outside 0 .. 2 550 000) is met with no index out of bounds: it raises the flag in the workspace, and
// `valid` says so.
#include <cmath>
#include "common.h"
#include "offgrid_cells.h"

namespace pcgc {
namespace {

constexpr double kGradMaxRadius = 16.0;             // |offset| <= 2^20; |dY| < 2^22, so a product is below 2^42
constexpr int kGradMaxK = 1 << 20;                  // ... and 2^20 terms stay inside int64
constexpr int kGradMaxY = 2550000;                  // 255 * (2126 + 7152 + 722)
constexpr double kGradScale = 65536.0;
constexpr double kGradDetFloor = 1e-6;

__global__ void __launch_bounds__(256) color_gradient_kernel(Target t, int64_t n, const float* normals, const int32_t* Y, double r2,
                                                             int kmin, double* grad, uint8_t* valid, int32_t* Kout, int64_t* Qout,
                                                             int64_t* Bout, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* g = t.q + i * 3;
  const double px = g[0], py = g[1], pz = g[2];
  const int32_t yi = Y[i];
  int K = 0;
  int64_t q00 = 0, q01 = 0, q02 = 0, q11 = 0, q12 = 0, q22 = 0, b0 = 0, b1 = 0, b2 = 0;
  bool dense = false;
  int cell[3];
  if (cell_of_point(t.c, g, cell) && yi >= 0 && yi <= kGradMaxY) {
    for_each_in_window(t, window_of(cell, 1, t.c.res), [&](int32_t j) {
      const float* q = t.q + (int64_t)j * 3;
      if (!(dist2(q, px, py, pz) <= r2)) return;           // false for a NaN
      if (K == kGradMaxK) {
        dense = true;
        return;
      }
      const int64_t a = llrint(((double)q[0] - px) * kGradScale);
      const int64_t b = llrint(((double)q[1] - py) * kGradScale);
      const int64_t c = llrint(((double)q[2] - pz) * kGradScale);
      // a neighbour's intensity outside the range raises the flag in its own thread; clamped here, it cannot overflow a sum
      const int64_t dy = (int64_t)min(max(Y[j], 0), kGradMaxY) - (int64_t)yi;
      ++K;
      q00 += a * a; q01 += a * b; q02 += a * c; q11 += b * b; q12 += b * c; q22 += c * c;
      b0 += a * dy; b1 += b * dy; b2 += c * dy;
    });
  } else {
    atomicOr(bad, kFlagInput);
  }
  if (dense) atomicOr(bad, kFlagDense);
  if (Kout) {
    Kout[i] = K;
    Qout[i * 6] = q00; Qout[i * 6 + 1] = q01; Qout[i * 6 + 2] = q02; Qout[i * 6 + 3] = q11; Qout[i * 6 + 4] = q12; Qout[i * 6 + 5] = q22;
    Bout[i * 3] = b0; Bout[i * 3 + 1] = b1; Bout[i * 3 + 2] = b2;
  }
  double* out = grad + i * 3;
  out[0] = 0.0; out[1] = 0.0; out[2] = 0.0;
  valid[i] = 0;
  const double n0 = (double)normals[i * 3], n1 = (double)normals[i * 3 + 1], n2 = (double)normals[i * 3 + 2];
  if (K < kmin || !(isfinite(n0) && isfinite(n1) && isfinite(n2)) || (n0 == 0.0 && n1 == 0.0 && n2 == 0.0)) return;
  // the tangent basis: e1 = (axis_k x n) / |axis_k x n| with k the axis of the smallest |n_k|, the first of equals; e2 = n x e1
  const double m0 = fabs(n0), m1 = fabs(n1), m2 = fabs(n2);
  const int k = m1 < m0 ? (m2 < m1 ? 2 : 1) : (m2 < m0 ? 2 : 0);
  const double c0 = k == 0 ? 0.0 : k == 1 ? n2 : -n1;
  const double c1 = k == 0 ? -n2 : k == 1 ? 0.0 : n0;
  const double c2 = k == 0 ? n1 : k == 1 ? -n0 : 0.0;
  const double len = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  const double e10 = c0 / len, e11 = c1 / len, e12 = c2 / len;
  const double e20 = n1 * e12 - n2 * e11, e21 = n2 * e10 - n0 * e12, e22 = n0 * e11 - n1 * e10;
  const double two32 = 4294967296.0;
  const double Q00 = (double)q00 / two32, Q01 = (double)q01 / two32, Q02 = (double)q02 / two32;
  const double Q11 = (double)q11 / two32, Q12 = (double)q12 / two32, Q22 = (double)q22 / two32;
  const double B0 = ((double)b0 / kGradScale) / (double)kGradMaxY, B1 = ((double)b1 / kGradScale) / (double)kGradMaxY;
  const double B2 = ((double)b2 / kGradScale) / (double)kGradMaxY;
  // u = Qd e1, v = Qd e2
  const double u0 = (Q00 * e10 + Q01 * e11) + Q02 * e12, u1 = (Q01 * e10 + Q11 * e11) + Q12 * e12, u2 = (Q02 * e10 + Q12 * e11) + Q22 * e12;
  const double v0 = (Q00 * e20 + Q01 * e21) + Q02 * e22, v1 = (Q01 * e20 + Q11 * e21) + Q12 * e22, v2 = (Q02 * e20 + Q12 * e21) + Q22 * e22;
  const double M00 = (e10 * u0 + e11 * u1) + e12 * u2, M01 = (e10 * v0 + e11 * v1) + e12 * v2, M11 = (e20 * v0 + e21 * v1) + e22 * v2;
  const double r0 = (e10 * B0 + e11 * B1) + e12 * B2, r1 = (e20 * B0 + e21 * B1) + e22 * B2;
  const double det = M00 * M11 - M01 * M01;
  const double tr = M00 + M11;
  if (!(det > kGradDetFloor * (tr * tr))) return;          // collinear neighbours (and a NaN)
  const double xa = (M11 * r0 - M01 * r1) / det, xb = (M00 * r1 - M01 * r0) / det;
  out[0] = xa * e10 + xb * e20;
  out[1] = xa * e11 + xb * e21;
  out[2] = xa * e12 + xb * e22;
  valid[i] = 1;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_color_gradient_workspace_bytes(int res, int64_t n) { return cloud_sizes_ok(res, n) ? cell_buffer_layout(res, n, nullptr).bytes : 0; }

int pcgc_color_gradient(const float* points, const float* normals, const int32_t* Y, int64_t n, double h, int ox, int oy, int oz, int res,
                        double radius, int kmin, double* g, uint8_t* valid, int32_t* K, int64_t* Q, int64_t* B, void* workspace,
                        size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && normals && Y && g && valid && workspace && cloud_sizes_ok(res, n) && grid_ok(h, ox, oy, oz, res, n, n),
               "pcgc_color_gradient: bad arguments");
  PCGC_REQUIRE((K != nullptr) == (Q != nullptr) && (K != nullptr) == (B != nullptr),
               "pcgc_color_gradient: K, Q and B come together or not at all");
  PCGC_REQUIRE(std::isfinite(radius) && radius > 0.0 && radius <= kGradMaxRadius && radius <= h,
               "pcgc_color_gradient: radius %g must be positive, at most %g and at most the cell edge %g", radius, kGradMaxRadius, h);
  PCGC_REQUIRE(kmin >= 3 && kmin <= kGradMaxK, "pcgc_color_gradient: kmin %d outside 3..%d", kmin, kGradMaxK);
  const CellBuffers b = cell_buffer_layout(res, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_color_gradient: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Target t;
  const int rc = build_cells(b.r, b.keys, b.start, b.bad, Cells{h, ox, oy, oz, res}, points, n, s, &t);
  if (rc) return rc;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(color_gradient_kernel, dim3(grid), dim3(256), 0, s, t, n, normals, Y, radius * radius, kmin, g, valid, K, Q, B, b.bad);
  hipLaunchKernelGGL(flag_marks_kernel, dim3(grid), dim3(256), 0, s, b.bad, n, valid);
  return launch_ok("colour gradient kernels");
}

}  // extern "C"
