// Steps 2 and 3 of the simplification rule (include/pcgc.h, pcgc_simplify_place): the quadric of a cluster and where it puts the
// cluster's vertex.  Kept free of HIP so that tests/surface_quadric_check.cpp can run it on the CPU against
// tests/_simplify_ref.py.  Float64 in the written order; the including files are built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include "jacobi3.h"

#if defined(__HIPCC__)
#define PCGC_QUADRIC_FN __device__ __forceinline__
#else
#define PCGC_QUADRIC_FN inline
#endif

namespace pcgc {
namespace {

constexpr double kQuadricRankEps = 1e-3;

// a00 a01 a02 a11 a12 a22 of A = sum n n^T, b = sum n d, and the sum of v - o over the cluster's vertices with their number
struct Quadric {
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double b[3] = {0.0, 0.0, 0.0};
  double sum[3] = {0.0, 0.0, 0.0};
  int64_t count = 0;
};

// o = (c + 0.5) * cell - 2 of the cluster with the key (cx * M + cy) * M + cz
PCGC_QUADRIC_FN void quadric_centre(int64_t key, int64_t M, int cell, double o[3]) {
  const int64_t c[3] = {key / (M * M), key / M % M, key % M};
  for (int j = 0; j < 3; ++j) o[j] = ((double)c[j] + 0.5) * (double)cell - 2.0;
}

// one triangle with the corners v0, v1, v2 (absolute), in the cluster centred on o
PCGC_QUADRIC_FN void quadric_add_triangle(Quadric& Q, const double o[3], const double v0[3], const double v1[3], const double v2[3]) {
  double q0[3], e1[3], e2[3];
  for (int j = 0; j < 3; ++j) {
    q0[j] = v0[j] - o[j];
    e1[j] = (v1[j] - o[j]) - q0[j];
    e2[j] = (v2[j] - o[j]) - q0[j];
  }
  const double nx = e1[1] * e2[2] - e1[2] * e2[1];
  const double ny = e1[2] * e2[0] - e1[0] * e2[2];
  const double nz = e1[0] * e2[1] - e1[1] * e2[0];
  const double d = -((nx * q0[0] + ny * q0[1]) + nz * q0[2]);
  Q.a[0] += nx * nx;
  Q.a[1] += nx * ny;
  Q.a[2] += nx * nz;
  Q.a[3] += ny * ny;
  Q.a[4] += ny * nz;
  Q.a[5] += nz * nz;
  Q.b[0] += nx * d;
  Q.b[1] += ny * d;
  Q.b[2] += nz * d;
}

PCGC_QUADRIC_FN void quadric_add_vertex(Quadric& Q, const double o[3], const double v[3]) {
  for (int j = 0; j < 3; ++j) Q.sum[j] += v[j] - o[j];
  ++Q.count;
}

// out = o + x; returns 1 where the cluster fell back to the mean (no positive eigenvalue, or the optimum left the cube)
PCGC_QUADRIC_FN int quadric_place(const Quadric& Q, const double o[3], int cell, double out[3]) {
  double m[3];
  for (int j = 0; j < 3; ++j) m[j] = Q.sum[j] / (double)Q.count;
  double A[3][3] = {{Q.a[0], Q.a[1], Q.a[2]}, {Q.a[1], Q.a[3], Q.a[4]}, {Q.a[2], Q.a[4], Q.a[5]}};
  double r[3];
  for (int i = 0; i < 3; ++i) r[i] = (-Q.b[i]) - ((A[i][0] * m[0] + A[i][1] * m[1]) + A[i][2] * m[2]);
  double E[3][3];
  jacobi3(A, E);
  const double lam[3] = {A[0][0], A[1][1], A[2][2]};
  const double lmax = fmax(fmax(lam[0], lam[1]), lam[2]);
  const double threshold = kQuadricRankEps * lmax;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i) {
    if (!(lam[i] > threshold)) continue;
    const double t = ((E[0][i] * r[0] + E[1][i] * r[1]) + E[2][i] * r[2]) / lam[i];
    for (int j = 0; j < 3; ++j) s[j] = s[j] + E[j][i] * t;
  }
  double x[3];
  int fallback = !(lmax > 0.0);
  for (int j = 0; j < 3; ++j) {
    x[j] = m[j] + s[j];
    if (fabs(x[j]) > (double)cell / 2.0) fallback = 1;
  }
  for (int j = 0; j < 3; ++j) out[j] = o[j] + (fallback ? m[j] : x[j]);
  return fallback;
}

}  // namespace
}  // namespace pcgc
