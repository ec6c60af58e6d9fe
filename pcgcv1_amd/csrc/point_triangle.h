// The squared distance from a point to a triangle (include/pcgc.h, pcgc_meshdist_query: "the rule"), in float64, one IEEE
// operation per written step.  Kept free of HIP so that tests/point_triangle_check.cpp can run it on the CPU against
// tests/_mesh_error_ref.py.  The including files are built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCGC_TRIANGLE_FN __device__ __forceinline__
#else
#define PCGC_TRIANGLE_FN inline
#endif

namespace pcgc {
namespace {

// The walk over the cells of a mesh (meshdist.hip) may end after the shell of half-width w cells once the best value found, or
// the squared gate, is below kShellKeep * (w h)^2.  Every triangle the walk has not met lies farther than R = w h from p in
// exact arithmetic, so it is enough that the VALUE the rule gives such a triangle stays above (1 - 2^-20) R^2:
//   * an edge term: w_k, e_k and r_k carry a few roundings of coordinates below 2^21, an absolute error below 2^-28 per
//     component (t e_k included: where t is not clipped, |s| <= l, and the error of s / l times |e| is a rounding of |w|),
//     so r.r >= (R - 2^-27)^2 (1 - 2^-50) >= R^2 (1 - 2^-25), R being at least 1 (w >= 1, h >= 1);
//   * the face term is the squared distance to the plane, which equals the distance to the triangle where the foot of p lies
//     inside and is smaller outside.  It counts outside only where rounding turned a side test, which puts the foot within
//     g <= 2^-49 |u| |v| / |b - a| of that side: the term is then R^2 - g^2 or more, above the bound for every triangle whose
//     sides are longer than 2^-38 of its distance from p.
// What the bound does not cover is a triangle whose computed normal is rounding noise alone (corners collinear to the last
// bit without being so exactly: exactly collinear corners in exactly representable positions, equal corners among them,
// give n = 0 and no face term): its face term is not tied to the geometry.  The factor leaves 2^5 of room over the edge terms.
constexpr double kShellKeep = 1.0 - 0x1p-20;

PCGC_TRIANGLE_FN void pt_sub(const double x[3], const double y[3], double d[3]) {
  d[0] = x[0] - y[0];
  d[1] = x[1] - y[1];
  d[2] = x[2] - y[2];
}

PCGC_TRIANGLE_FN double pt_dot(const double x[3], const double y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

PCGC_TRIANGLE_FN void pt_cross(const double x[3], const double y[3], double c[3]) {
  c[0] = x[1] * y[2] - x[2] * y[1];
  c[1] = x[2] * y[0] - x[0] * y[2];
  c[2] = x[0] * y[1] - x[1] * y[0];
}

PCGC_TRIANGLE_FN double pt_min(double x, double y) { return x < y ? x : y; }

// seg(p, u, v): the squared distance from p to the segment u v; a segment of length zero is the point u
PCGC_TRIANGLE_FN double pt_segment_d2(const double p[3], const double u[3], const double v[3]) {
  double e[3], w[3], r[3];
  pt_sub(v, u, e);
  pt_sub(p, u, w);
  const double l = pt_dot(e, e), s = pt_dot(w, e);
  double t = 0.0;
  if (l > 0.0) {
    t = s / l;
    if (t < 0.0) t = 0.0;
    if (t > 1.0) t = 1.0;
  }
  r[0] = w[0] - t * e[0];
  r[1] = w[1] - t * e[1];
  r[2] = w[2] - t * e[2];
  return pt_dot(r, r);
}

// d2(p, (a, b, c))
PCGC_TRIANGLE_FN double point_triangle_d2(const double p[3], const double a[3], const double b[3], const double c[3]) {
  double d = pt_min(pt_segment_d2(p, a, b), pt_segment_d2(p, b, c));
  d = pt_min(d, pt_segment_d2(p, c, a));
  double ab[3], ac[3], n[3];
  pt_sub(b, a, ab);
  pt_sub(c, a, ac);
  pt_cross(ab, ac, n);
  const double nn = pt_dot(n, n);
  if (!(nn > 0.0)) return d;
  double u[3], v[3], w[3], x[3];
  pt_sub(a, p, u);
  pt_sub(b, p, v);
  pt_sub(c, p, w);
  pt_cross(u, v, x);
  if (!(pt_dot(n, x) >= 0.0)) return d;
  pt_cross(v, w, x);
  if (!(pt_dot(n, x) >= 0.0)) return d;
  pt_cross(w, u, x);
  if (!(pt_dot(n, x) >= 0.0)) return d;
  double pa[3];
  pt_sub(p, a, pa);
  const double dn = pt_dot(n, pa);
  return pt_min(d, dn * dn / nn);
}

}  // namespace
}  // namespace pcgc
