// Stand-alone: runs pcgcv1_amd/csrc/point_triangle.h (the point-to-triangle rule of include/pcgc.h, what meshdist.hip measures
// a candidate with) on the pairs it reads from standard input and prints, per pair, the squared distance as a hex float.  Input,
// numbers as hex floats: the number of pairs, then per pair the point and the three corners (twelve numbers).
// tests/test_mesh_error_host.py compares with tests/_mesh_error_ref.py: d2.
#include <cstdio>

#include "../pcgcv1_amd/csrc/point_triangle.h"

static bool read3(double* v) { return std::scanf("%la %la %la", v, v + 1, v + 2) == 3; }

int main() {
  int n = 0;
  if (std::scanf("%d", &n) != 1) return 2;
  for (int k = 0; k < n; ++k) {
    double p[3], a[3], b[3], c[3];
    if (!read3(p) || !read3(a) || !read3(b) || !read3(c)) return 2;
    std::printf("%a\n", pcgc::point_triangle_d2(p, a, b, c));
  }
  return 0;
}
