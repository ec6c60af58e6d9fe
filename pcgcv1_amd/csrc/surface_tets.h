// The marching-tetrahedra rule of surface.hip (include/pcgc.h, pcgc_surface_triangles), kept free of HIP so that
// tests/surface_tets_check.cpp can run it on the CPU against tests/_surface_ref.py.
//
// Corner o of a cell is bit (ox << 2 | oy << 1 | oz) of `inside`.  The Kuhn tetrahedron of the permutation (a0, a1, a2) of the
// axes has the corners 0, e_a0, e_a0 + e_a1, 7: a chain in which every corner contains the one before, so the ends of an edge
// order as their positions in the tetrahedron do.
#pragma once

#if defined(__HIPCC__)
#define PCGC_TETS_FN __host__ __device__ __forceinline__
#else
#define PCGC_TETS_FN inline
#endif

namespace pcgc {

// direction index of an edge from the bits its upper corner adds: 100 010 001 110 101 011 111 -> 0 .. 6
PCGC_TETS_FN int direction_of(int diff) {
  switch (diff & 7) {
    case 4: return 0;
    case 2: return 1;
    case 1: return 2;
    case 6: return 3;
    case 5: return 4;
    case 3: return 5;
    default: return 6;
  }
}

// the corner bits a direction index adds
PCGC_TETS_FN int direction_bits(int dir) {
  switch (dir) {
    case 0: return 4;
    case 1: return 2;
    case 2: return 1;
    case 3: return 6;
    case 4: return 5;
    case 5: return 3;
    default: return 7;
  }
}

// first and second axis of permutation t in lexicographic (itertools.permutations) order, and its sign
PCGC_TETS_FN int perm_first(int t) { return t >> 1; }
PCGC_TETS_FN int perm_second(int t) {
  const int a = t >> 1, lower = (t & 1) == 0;       // the two axes left, ascending; an even t takes the lower
  const int r0 = a == 0 ? 1 : 0, r1 = a == 2 ? 1 : 2;
  return lower ? r0 : r1;
}
PCGC_TETS_FN int perm_sign(int t) { return (t == 0 || t == 3 || t == 4) ? 1 : -1; }

// emit(e0, e1, e2) for every triangle of the cell's six tetrahedra, in the rule's order and winding; an edge is
// (lower corner << 3 | upper corner)
template <typename F>
PCGC_TETS_FN void cell_triangles(unsigned inside, F emit) {
  for (int t = 0; t < 6; ++t) {
    int corner[4];
    corner[0] = 0;
    corner[1] = 4 >> perm_first(t);
    corner[2] = corner[1] | (4 >> perm_second(t));
    corner[3] = 7;
    int I[4], O[4], ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
      if ((inside >> corner[i]) & 1u) I[ni++] = i; else O[no++] = i;
    }
    if (ni == 0 || ni == 4) continue;
    int inv = 0;                                     // inversions of the sequence (inside corners, outside corners)
    for (int a = 0; a < ni; ++a)
      for (int b = 0; b < no; ++b) inv += O[b] < I[a];
    const bool flip = (perm_sign(t) < 0) != ((inv & 1) != 0);
    auto edge = [&](int u, int v) { return u < v ? (corner[u] << 3 | corner[v]) : (corner[v] << 3 | corner[u]); };
    if (ni == 1) {
      const int e0 = edge(I[0], O[0]), e1 = edge(I[0], O[1]), e2 = edge(I[0], O[2]);
      if (flip) emit(e0, e2, e1); else emit(e0, e1, e2);
    } else if (ni == 3) {
      const int e0 = edge(I[0], O[0]), e1 = edge(I[1], O[0]), e2 = edge(I[2], O[0]);
      if (flip) emit(e0, e2, e1); else emit(e0, e1, e2);
    } else {
      const int A = edge(I[0], O[0]), B = edge(I[0], O[1]), C = edge(I[1], O[1]), D = edge(I[1], O[0]);
      if (flip) { emit(A, C, B); emit(A, D, C); } else { emit(A, B, C); emit(A, C, D); }
    }
  }
}

}  // namespace pcgc
