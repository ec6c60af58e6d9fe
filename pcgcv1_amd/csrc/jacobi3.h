// The symmetric 3x3 eigen-solver the normal estimation (mesh.hip) and the scan smoothing (smooth.hip) share: one copy, so that
// both follow the same operations in the same order.  The including files are built with -ffp-contract=off; tests/_smooth_ref.py
// restates the loop in numpy operation for operation.  Internal linkage: the objects link into one library.  Without hipcc
// (tests/surface_quadric_check.cpp, through surface_quadric.h) the same text is a host function.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#include "common.h"
#define PCGC_JACOBI_FN __device__
#else
#define PCGC_JACOBI_FN inline
#endif

namespace pcgc {
namespace {

// cyclic Jacobi on the symmetric 3x3 a (destroyed): eigenvalues on the diagonal, eigenvectors in the columns of v
PCGC_JACOBI_FN void jacobi3(double a[3][3], double v[3][3]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double g = 100.0 * fabs(apq);
      if (sweep > 3 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
        a[p][q] = a[q][p] = 0.0;                 // below the diagonal's precision
        continue;
      }
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      for (int k = 0; k < 3; ++k) {              // a <- a J (columns p, q)
        const double akp = a[k][p], akq = a[k][q];
        a[k][p] = c * akp - s * akq;
        a[k][q] = s * akp + c * akq;
      }
      for (int k = 0; k < 3; ++k) {              // a <- J^T a (rows p, q)
        const double apk = a[p][k], aqk = a[q][k];
        a[p][k] = c * apk - s * aqk;
        a[q][k] = s * apk + c * aqk;
      }
      a[p][q] = a[q][p] = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
      }
    }
  }
}

}  // namespace
}  // namespace pcgc
