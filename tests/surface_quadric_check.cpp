// Stand-alone: runs pcgcv1_amd/csrc/surface_quadric.h (steps 2 and 3 of the simplification rule, what simplify.hip places a
// cluster's vertex with) on the clusters it reads from standard input and prints, per cluster, the placed vertex as three hex
// floats and the fallback flag.  Input, numbers as hex floats: the number of clusters, then per cluster "cell nv nt", the centre,
// nv vertices (three numbers each) and nt triangles (nine numbers each: the three corners).  tests/test_simplify_host.py compares
// with tests/_simplify_ref.py: place_clusters.
#include <cstdio>

#include "../pcgcv1_amd/csrc/surface_quadric.h"

static bool read3(double* v) { return std::scanf("%la %la %la", v, v + 1, v + 2) == 3; }

int main() {
  int n = 0;
  if (std::scanf("%d", &n) != 1) return 2;
  for (int k = 0; k < n; ++k) {
    int cell = 0, nv = 0, nt = 0;
    double o[3], v[3][3];
    if (std::scanf("%d %d %d", &cell, &nv, &nt) != 3 || !read3(o)) return 2;
    pcgc::Quadric Q;
    for (int i = 0; i < nv; ++i) {
      if (!read3(v[0])) return 2;
      pcgc::quadric_add_vertex(Q, o, v[0]);
    }
    for (int i = 0; i < nt; ++i) {
      if (!read3(v[0]) || !read3(v[1]) || !read3(v[2])) return 2;
      pcgc::quadric_add_triangle(Q, o, v[0], v[1], v[2]);
    }
    double out[3];
    const int fallback = pcgc::quadric_place(Q, o, cell, out);
    std::printf("%a %a %a %d\n", out[0], out[1], out[2], fallback);
  }
  return 0;
}
