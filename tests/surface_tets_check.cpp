// Stand-alone: prints what pcgcv1_amd/csrc/surface_tets.h (the marching-tetrahedra rule of surface.hip) gives for every one of
// the 256 inside patterns of a cell, one line each: "<inside> <e0> <e1> <e2> ...", three edges per triangle, and a last line
// "dir" with direction_of(1 .. 7) and direction_bits(0 .. 6).  tests/test_surface_host.py compares with tests/_surface_ref.py.
#include <cstdio>

#include "../pcgcv1_amd/csrc/surface_tets.h"

int main() {
  for (unsigned inside = 0; inside < 256; ++inside) {
    std::printf("%u", inside);
    pcgc::cell_triangles(inside, [](int e0, int e1, int e2) { std::printf(" %d %d %d", e0, e1, e2); });
    std::printf("\n");
  }
  std::printf("dir");
  for (int d = 1; d < 8; ++d) std::printf(" %d", pcgc::direction_of(d));
  for (int d = 0; d < 7; ++d) std::printf(" %d", pcgc::direction_bits(d));
  std::printf("\n");
  return 0;
}
