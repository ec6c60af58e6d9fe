// Quadric vertex clustering of a triangle mesh (gfx950): what pcgcv1_amd/surface.py simplifies with.
//
// include/pcgc.h states the rule (tests/_simplify_ref.py restates it in numpy).  torch sorts, uniques and searches
// (the canonical order of the triangles, the distinct cluster keys, the incidence words, the triples); the kernels are
//   * simplify_keys_kernel: one thread per vertex, its cluster key;
//   * simplify_incidence_kernel: one thread per triangle, three words: the cluster rank of each corner, or K where an earlier
//     corner of the triangle has that cluster already.  A stable sort of the words keeps the canonical order inside each run;
//   * simplify_place_kernel: one thread per cluster walks its run of the sorted incidence list and its vertices in order, sums
//     the quadric and the mean in float64 (surface_quadric.h, this file is built with -ffp-contract=off), solves and writes the
//     vertex and a fallback flag.  A gather through two levels of indices: the triangle of the next entry is fetched while the
//     corners of this one are in flight, and many clusters per SIMD hide the rest;
//   * simplify_remap_kernel: one thread per triangle, the unoriented triple of cluster ranks (or the degenerate mark), its sign
//     and, where three ranks fit 63 bits, the packed triple.
// No atomics at all: two calls give the same bytes.  Every index read from the caller's arrays is checked before it is used.
#include "common.h"
#include "surface_quadric.h"

namespace pcgc {
namespace {

constexpr int kSimpThreads = 256, kSimpMaxBits = 12, kSimpMaxCell = 64, kSimpPackBits = 21;

unsigned simp_blocks(int64_t n) { return (unsigned)((n + kSimpThreads - 1) / kSimpThreads); }

bool simp_grid_ok(int bits, int cell) { return bits >= 1 && bits <= kSimpMaxBits && cell >= 1 && cell <= kSimpMaxCell; }

int64_t simp_side(int bits, int cell) { return (((int64_t)1 << bits) + 4 + cell - 1) / cell; }

__global__ void __launch_bounds__(kSimpThreads) simplify_keys_kernel(const double* v, int64_t n, double hi, int cell, int64_t M, int64_t* keys) {
  const int64_t i = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
  if (i >= n) return;
  int64_t key = 0;
  bool ok = true;
  for (int j = 0; j < 3; ++j) {
    const double x = v[i * 3 + j];
    ok = ok && x >= -2.0 && x < hi;                                    // false for a NaN
    const int64_t c = ok ? (int64_t)floor((x + 2.0) / (double)cell) : 0;
    key = key * M + c;
  }
  keys[i] = ok ? key : -1;
}

// rank of corner j of triangle t, or -1 where the index leaves the vertices or the rank the clusters
__device__ __forceinline__ int64_t corner_rank(const int32_t* tri, int64_t t, int j, const int32_t* rank, int64_t V, int64_t K) {
  const int32_t i = tri[t * 3 + j];
  if (i < 0 || i >= V) return -1;
  const int32_t r = rank[i];
  return r < 0 || r >= K ? -1 : r;
}

__global__ void __launch_bounds__(kSimpThreads) simplify_incidence_kernel(const int32_t* tri, int64_t T, const int32_t* rank, int64_t V, int64_t K,
                                                                         int32_t* words) {
  const int64_t t = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
  if (t >= T) return;
  const int64_t a = corner_rank(tri, t, 0, rank, V, K), b = corner_rank(tri, t, 1, rank, V, K), c = corner_rank(tri, t, 2, rank, V, K);
  words[t * 3] = (int32_t)(a < 0 ? K : a);
  words[t * 3 + 1] = (int32_t)(b < 0 || b == a ? K : b);
  words[t * 3 + 2] = (int32_t)(c < 0 || c == a || c == b ? K : c);
}

struct Corners {
  int32_t i[3];
};

__device__ __forceinline__ Corners load_corners(const int32_t* tri, int64_t T, const int64_t* entry, int64_t at, int64_t end) {
  Corners c = {{-1, -1, -1}};
  if (at < end) {
    const int64_t e = entry[at];
    if (e >= 0 && e < T * 3) {
      const int64_t t = e / 3;
      c.i[0] = tri[t * 3];
      c.i[1] = tri[t * 3 + 1];
      c.i[2] = tri[t * 3 + 2];
    }
  }
  return c;
}

__global__ void __launch_bounds__(kSimpThreads) simplify_place_kernel(const double* v, int64_t V, const int32_t* tri, int64_t T,
                                                                     const int64_t* cluster_keys, int64_t K, int cell, int64_t M,
                                                                     const int64_t* tri_start, const int64_t* tri_entry,
                                                                     const int64_t* vert_start, const int64_t* vert_index, double* placed,
                                                                     uint8_t* fallback) {
  const int64_t k = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
  if (k >= K) return;
  double o[3];
  quadric_centre(cluster_keys[k], M, cell, o);
  Quadric Q;
  const int64_t v0 = max((int64_t)0, vert_start[k]), v1 = min(V, vert_start[k + 1]);
  for (int64_t at = v0; at < v1; ++at) {
    const int64_t i = vert_index[at];
    if (i < 0 || i >= V) continue;
    const double p[3] = {v[i * 3], v[i * 3 + 1], v[i * 3 + 2]};
    quadric_add_vertex(Q, o, p);
  }
  const int64_t t0 = max((int64_t)0, tri_start[k]), t1 = min(T * 3, tri_start[k + 1]);
  Corners next = load_corners(tri, T, tri_entry, t0, t1);
  for (int64_t at = t0; at < t1; ++at) {
    const Corners c = next;
    next = load_corners(tri, T, tri_entry, at + 1, t1);
    if (c.i[0] < 0 || c.i[0] >= V || c.i[1] < 0 || c.i[1] >= V || c.i[2] < 0 || c.i[2] >= V) continue;
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double* src = v + (int64_t)c.i[j] * 3;
      p[j][0] = src[0];
      p[j][1] = src[1];
      p[j][2] = src[2];
    }
    quadric_add_triangle(Q, o, p[0], p[1], p[2]);
  }
  double out[3] = {o[0], o[1], o[2]};
  int fb = 1;
  if (Q.count > 0) fb = quadric_place(Q, o, cell, out);
  placed[k * 3] = out[0];
  placed[k * 3 + 1] = out[1];
  placed[k * 3 + 2] = out[2];
  fallback[k] = (uint8_t)fb;
}

__global__ void __launch_bounds__(kSimpThreads) simplify_remap_kernel(const int32_t* tri, int64_t T, const int32_t* rank, int64_t V, int64_t K,
                                                                     int32_t* triples, int32_t* sign, int64_t* packed) {
  const int64_t t = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
  if (t >= T) return;
  const int64_t r[3] = {corner_rank(tri, t, 0, rank, V, K), corner_rank(tri, t, 1, rank, V, K), corner_rank(tri, t, 2, rank, V, K)};
  const bool degenerate = r[0] < 0 || r[1] < 0 || r[2] < 0 || r[0] == r[1] || r[1] == r[2] || r[0] == r[2];
  int64_t a = -1, lo = -1, hi = -1;
  int sg = 0;
  if (!degenerate) {
    const int first = r[0] < r[1] ? (r[0] < r[2] ? 0 : 2) : (r[1] < r[2] ? 1 : 2);
    a = r[first];
    const int64_t b = r[(first + 1) % 3], c = r[(first + 2) % 3];
    sg = b < c ? 1 : -1;
    lo = b < c ? b : c;
    hi = b < c ? c : b;
  }
  triples[t * 3] = (int32_t)a;
  triples[t * 3 + 1] = (int32_t)lo;
  triples[t * 3 + 2] = (int32_t)hi;
  sign[t] = sg;
  if (packed) packed[t] = degenerate ? -1 : (a << (2 * kSimpPackBits) | lo << kSimpPackBits | hi);
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_simplify_keys(const double* vertices, int64_t n_vertices, int bits, int cell, int64_t* keys, pcgc_stream_t stream) {
  PCGC_REQUIRE(vertices && keys && n_vertices >= 1 && n_vertices <= 0x7FFFFFFF && simp_grid_ok(bits, cell),
               "pcgc_simplify_keys: bad arguments (bits 1..%d, cell 1..%d)", kSimpMaxBits, kSimpMaxCell);
  hipLaunchKernelGGL(simplify_keys_kernel, dim3(simp_blocks(n_vertices)), dim3(kSimpThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     (double)((1 << bits) + 2), cell, simp_side(bits, cell), keys);
  return launch_ok("simplify_keys_kernel");
}

int pcgc_simplify_incidence(const int32_t* triangles, int64_t n_triangles, const int32_t* rank, int64_t n_vertices, int64_t n_clusters,
                            int32_t* words, pcgc_stream_t stream) {
  PCGC_REQUIRE(triangles && rank && words && n_triangles >= 1 && n_triangles <= 0x7FFFFFFF / 3 && n_vertices >= 1 &&
                   n_vertices <= 0x7FFFFFFF && n_clusters >= 1 && n_clusters <= n_vertices,
               "pcgc_simplify_incidence: bad arguments");
  hipLaunchKernelGGL(simplify_incidence_kernel, dim3(simp_blocks(n_triangles)), dim3(kSimpThreads), 0, (hipStream_t)stream, triangles,
                     n_triangles, rank, n_vertices, n_clusters, words);
  return launch_ok("simplify_incidence_kernel");
}

int pcgc_simplify_place(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                        const int64_t* cluster_keys, int64_t n_clusters, int bits, int cell, const int64_t* tri_start,
                        const int64_t* tri_entry, const int64_t* vert_start, const int64_t* vert_index, double* placed, uint8_t* fallback,
                        pcgc_stream_t stream) {
  PCGC_REQUIRE(vertices && cluster_keys && vert_start && vert_index && tri_start && placed && fallback && n_vertices >= 1 &&
                   n_vertices <= 0x7FFFFFFF && n_triangles >= 0 && n_triangles <= 0x7FFFFFFF / 3 && n_clusters >= 1 &&
                   n_clusters <= n_vertices && simp_grid_ok(bits, cell) && (n_triangles == 0 || (triangles && tri_entry)),
               "pcgc_simplify_place: bad arguments (bits 1..%d, cell 1..%d)", kSimpMaxBits, kSimpMaxCell);
  hipLaunchKernelGGL(simplify_place_kernel, dim3(simp_blocks(n_clusters)), dim3(kSimpThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     triangles, n_triangles, cluster_keys, n_clusters, cell, simp_side(bits, cell), tri_start, tri_entry, vert_start, vert_index,
                     placed, fallback);
  return launch_ok("simplify_place_kernel");
}

int pcgc_simplify_remap(const int32_t* triangles, int64_t n_triangles, const int32_t* rank, int64_t n_vertices, int64_t n_clusters,
                        int32_t* triples, int32_t* sign, int64_t* packed, pcgc_stream_t stream) {
  PCGC_REQUIRE(triangles && rank && triples && sign && n_triangles >= 1 && n_triangles <= 0x7FFFFFFF / 3 && n_vertices >= 1 &&
                   n_vertices <= 0x7FFFFFFF && n_clusters >= 1 && n_clusters <= n_vertices,
               "pcgc_simplify_remap: bad arguments");
  PCGC_REQUIRE(!packed || n_clusters <= ((int64_t)1 << kSimpPackBits), "pcgc_simplify_remap: %lld clusters do not pack into 63 bits",
               (long long)n_clusters);
  hipLaunchKernelGGL(simplify_remap_kernel, dim3(simp_blocks(n_triangles)), dim3(kSimpThreads), 0, (hipStream_t)stream, triangles, n_triangles,
                     rank, n_vertices, n_clusters, triples, sign, packed);
  return launch_ok("simplify_remap_kernel");
}

}  // extern "C"
