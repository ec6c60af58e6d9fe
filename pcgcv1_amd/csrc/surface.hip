// A triangle mesh from a voxel cloud (gfx950): what pcgcv1_amd/surface.py reconstructs with.
//
// include/pcgc.h states the rule (tests/_surface_ref.py restates it in numpy).  Three parts, all on voxel_grid.h's
// bit set with its rank table, float64 sums in a fixed order (this file is built with -ffp-contract=off):
//   * orientation: Jacobi rounds over the link graph (Chebyshev distance <= G).  One thread per voxel per round, the signs in two
//     buffers indexed by rank (a round reads one and writes the other), the neighbours read as masked words of the bit set the
//     way components.hip reads its columns.  The stage, the round count and the "set something / unset remain" word live in
//     device memory: surface_tail_kernel, one thread, advances them after every round, and a round that finds `done` set
//     returns at once, so the host queues a batch of rounds per read-back of that word;
//   * the lattice: two more bit sets, the candidate cells over (res + 2)^3 and the lattice vertices over (res + 3)^3, marked
//     from the voxels as z-runs (one or two atomicOr per run), scanned with the popcount scan; the vertices get a rank table.
//     surface_implicit_kernel, one thread per vertex, walks its (2R + 2)^2 columns of the occupancy bit set in ascending
//     offset order: two float64 accumulators, a normal load only on a hit, no atomics;
//   * marching tetrahedra: surface_triangles_kernel walks the cell bit set (every thread its words of a scan block), counts
//     or emits the triangles of the six Kuhn tetrahedra of each cell as lattice-edge ids; block_scan and
//     grid_block_scan_kernel place them.  The host sorts and uniques the ids (plumbing); surface_vertices_kernel places a
//     vertex per id and surface_index_kernel turns ids into indices with find_sorted_key.
// The winding of a triangle comes from the parity of the tetrahedron and of its inside corners, never from a float test.
// Integer atomics only (atomicOr on bit sets and on the flag word): two calls give the same bytes.
#include <algorithm>
#include "common.h"
#include "voxel_grid.h"
#include "surface_tets.h"      // cell_triangles, direction_of, direction_bits

namespace pcgc {
namespace {

constexpr int kSurfMaxBits = 12, kSurfMaxGap = 8, kSurfMinRadius = 3, kSurfMaxRadius = 8, kSurfMaxStages = 8;
constexpr int kSurfThreads = 256;

// the words the rounds and their tail share
struct OrientState {
  int stage;        // index into tau
  unsigned flags;   // bit 0: this round set a voxel, bit 1: a voxel is still unset
  int rounds;       // rounds run so far
  int done;         // 0 running, 1 every voxel set, 2 a component has no seed (nothing can be set at the last stage)
};

struct Tau {
  double v[kSurfMaxStages];
  int n;
};

__device__ __forceinline__ void flag_wave(OrientState* st, int fl) {
  const unsigned long long set = __ballot(fl == 1), unset = __ballot(fl == 2);
  if ((threadIdx.x & 63) != 0 || !(set | unset)) return;
  // thousands of waves raise the same two bits of one word: look first (past the L1, as components.hip reads its parents), so that
  // all but the first few skip the atomic; a stale look costs one atomic more, never a bit
  const unsigned want = (set ? 1u : 0u) | (unset ? 2u : 0u);
  if ((__hip_atomic_load(&st->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & want) != want) atomicOr(&st->flags, want);
}

// order[rank of the cell of row i] = i: the rows in key order
__global__ void __launch_bounds__(kSurfThreads) surface_order_kernel(const int32_t* p, int64_t n, int res, const unsigned* bits,
                                                                    const unsigned* rank, unsigned* order) {
  const int64_t i = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  if (in_grid(res, x, y, z)) order[rank_of(bits, rank, cell_of(res, x, y, z))] = (unsigned)i;
}

// sign of every rank before the first round: a seed takes the sign of its x component, the rest are unset (0)
__global__ void __launch_bounds__(kSurfThreads) surface_seed_kernel(const float* normals, const uint8_t* seed, const unsigned* order,
                                                                   const int64_t* n_set, int8_t* sign, OrientState* st) {
  const int64_t r = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  int fl = 0;
  if (r < *n_set) {
    const unsigned i = order[r];
    const int8_t s = seed[i] ? (normals[(int64_t)i * 3] < 0.0f ? -1 : 1) : 0;
    sign[r] = s;
    fl = s == 0 ? 2 : 0;
  }
  flag_wave(st, fl);
}

// after the seeds (count == 0) and after every round (count == 1)
__global__ void surface_tail_kernel(OrientState* st, int n_tau, int count) {
  if (st->done) return;
  const unsigned f = st->flags;
  st->flags = 0;
  if (count) {
    st->rounds += 1;
    st->stage = (f & 1u) ? 0 : st->stage + 1;
  }
  if (!(f & 2u)) st->done = 1;
  else if (st->stage >= n_tau) st->done = 2;
}

__global__ void __launch_bounds__(kSurfThreads) surface_round_kernel(const int32_t* p, const float* normals, const unsigned* order,
                                                                    const int64_t* n_set, int bits_per_axis, int G, const unsigned* bits,
                                                                    const unsigned* rank, Tau tau, const int8_t* in, int8_t* out,
                                                                    OrientState* st) {
  if (st->done) return;
  const int64_t r = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  int fl = 0;
  if (r < *n_set) {
    int8_t s = in[r];
    if (s == 0) {
      const int res = 1 << bits_per_axis;
      const int64_t i = order[r];
      const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
      const double nx = normals[i * 3], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
      const int64_t own = cell_of(res, x, y, z);
      double best = -1.0, best_c = 0.0;
      int best_s = 0;
      for (int dx = -G; dx <= G; ++dx)
        for (int dy = -G; dy <= G; ++dy) {
          const int qx = x + dx, qy = y + dy;
          if ((unsigned)qx >= (unsigned)res || (unsigned)qy >= (unsigned)res) continue;
          const int z0 = max(z - G, 0), z1 = min(z + G, res - 1);
          const int64_t row = cell_of(res, qx, qy, 0);
          for_each_in_run(bits, row + z0, row + z1, [&](int64_t w, unsigned all, int b) {
            if ((w << 5) + b == own) return;
            const int64_t jr = (int64_t)rank[w] + __popc(all & ((1u << b) - 1u));
            const int sj = in[jr];
            if (sj == 0) return;
            const int64_t j = order[jr];
            const double c = (nx * (double)normals[j * 3] + ny * (double)normals[j * 3 + 1]) + nz * (double)normals[j * 3 + 2];
            const double a = fabs(c);
            if (a > best) { best = a; best_c = c; best_s = sj; }         // ascending keys: the first of equal |c| stays
          });
        }
      if (best >= tau.v[st->stage]) {
        s = (int8_t)(best_c >= 0.0 ? best_s : -best_s);
        fl = 1;
      } else {
        fl = 2;
      }
    }
    out[r] = s;
  }
  flag_wave(st, fl);
}

// per input row; a row outside the grid gets 0
__global__ void __launch_bounds__(kSurfThreads) surface_sign_gather_kernel(const int32_t* p, int64_t n, int res, const unsigned* bits,
                                                                          const unsigned* rank, const int8_t* sign, int8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  out[i] = in_grid(res, x, y, z) ? sign[rank_of(bits, rank, cell_of(res, x, y, z))] : (int8_t)0;
}

// ------------------------------------------------------------------------------------------------------------------ the lattice
// len <= 4 consecutive bits from b0 on
__device__ __forceinline__ void set_run(unsigned* bits, int64_t b0, int len) {
  const int64_t w = b0 >> 5;
  const int sh = (int)(b0 & 31);
  const unsigned run = (1u << len) - 1u;
  atomicOr(&bits[w], run << sh);
  if (sh + len > 32) atomicOr(&bits[w + 1], run >> (32 - sh));
}

// Cell c in [-1, res]^3 is bit c + 1 of the (res + 2)^3 set, vertex k in [-2, res]^3 bit k + 2 of the (res + 3)^3 set.  A voxel
// q marks the cells q + {-1, 0, 1}^3, bits q + {0, 1, 2}^3, and their corners q + {-2 .. 1}^3, bits q + {0 .. 3}^3.
__global__ void __launch_bounds__(kSurfThreads) surface_mark_kernel(const int32_t* p, int64_t n, int res, unsigned* cbits, unsigned* vbits) {
  const int64_t i = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  if (!in_grid(res, x, y, z)) return;
  for (int dx = 0; dx < 3; ++dx)
    for (int dy = 0; dy < 3; ++dy) set_run(cbits, cell_of(res + 2, x + dx, y + dy, z), 3);
  for (int dx = 0; dx < 4; ++dx)
    for (int dy = 0; dy < 4; ++dy) set_run(vbits, cell_of(res + 3, x + dx, y + dy, z), 4);
}

__global__ void surface_counts_kernel(const int64_t* n_cells, const int64_t* n_vertices, int64_t* counts) {
  counts[0] = *n_cells;
  counts[1] = *n_vertices;
}

__global__ void __launch_bounds__(kScanThreads) surface_vertex_list_kernel(const unsigned* vbits, const int64_t* block_offset, int64_t n_vertices,
                                                                           int64_t* vkeys) {
  for_each_set_bit(vbits, block_offset, [&](int64_t o, int64_t k) {
    if (o < n_vertices) vkeys[o] = k;
  });
}

// oriented normals in key order
__global__ void __launch_bounds__(kSurfThreads) surface_normals_kernel(const double* N, const unsigned* order, const int64_t* n_set,
                                                                      double* sorted) {
  const int64_t r = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (r >= *n_set) return;
  const int64_t i = order[r];
  sorted[r * 3] = N[i * 3];
  sorted[r * 3 + 1] = N[i * 3 + 1];
  sorted[r * 3 + 2] = N[i * 3 + 2];
}

// The vertex stands at k + 0.5; with q = k + o the doubled offset (2k + 1) - 2q is 1 - 2o, whatever k.
__global__ void __launch_bounds__(kSurfThreads) surface_implicit_kernel(const int64_t* vkeys, int64_t n_vertices, const int64_t* vn_set, int res,
                                                                       int R, const unsigned* bits, const unsigned* rank, const double* N,
                                                                       double* f) {
  const int64_t v = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (v >= n_vertices || v >= *vn_set) return;
  const int64_t side = res + 3, key = vkeys[v];
  const int kx = (int)(key / (side * side)) - 2, ky = (int)(key / side % side) - 2, kz = (int)(key % side) - 2;
  const int lim = 4 * R * R;
  const double denom = (double)(lim + 1);
  double num = 0.0, W = 0.0;
  for (int ox = -R; ox <= R + 1; ++ox)
    for (int oy = -R; oy <= R + 1; ++oy) {
      const int ddx = 1 - 2 * ox, ddy = 1 - 2 * oy;
      const int dxy = ddx * ddx + ddy * ddy;
      const int qx = kx + ox, qy = ky + oy;
      if (dxy > lim || (unsigned)qx >= (unsigned)res || (unsigned)qy >= (unsigned)res) continue;
      const int z0 = max(kz - R, 0), z1 = min(kz + R + 1, res - 1);
      if (z1 < z0) continue;
      const int64_t row = cell_of(res, qx, qy, 0);
      for_each_in_run(bits, row + z0, row + z1, [&](int64_t w, unsigned all, int b) {
        const int ddz = 1 - 2 * ((int)((w << 5) + b - row) - kz);
        const int d2 = dxy + ddz * ddz;
        if (d2 > lim) return;
        const double* Nq = N + 3 * ((int64_t)rank[w] + __popc(all & ((1u << b) - 1u)));
        const double t = 1.0 - (double)d2 / denom;
        const double wt = t * t;
        num += wt * ((Nq[0] * (double)ddx + Nq[1] * (double)ddy) + Nq[2] * (double)ddz);
        W += wt;
      });
    }
  f[v] = 0.5 * num / W;
}

// ------------------------------------------------------------------------------------------------------------------ tetrahedra
struct Lattice {
  const unsigned* vbits;
  const unsigned* vrank;
  const double* f;
  int64_t n_vertices;
  int side;         // res + 3
};

// f at the vertex with padded coordinates (x, y, z); +0.0 (outside) where the lattice holds none, which a coherent call never asks
__device__ __forceinline__ double f_at(const Lattice& L, int x, int y, int z) {
  if (!in_grid(L.side, x, y, z)) return 0.0;
  const int64_t idx = cell_of(L.side, x, y, z);
  if (!((L.vbits[idx >> 5] >> (idx & 31)) & 1u)) return 0.0;
  const int64_t r = rank_of(L.vbits, L.vrank, idx);
  return r < L.n_vertices ? L.f[r] : 0.0;
}

// f(cx, cy, cz, inside) for every cell among the calling thread's words w of scan block blockIdx.x that the surface crosses, in
// key order.  The cell's padded coordinates are its lowest corner's padded vertex coordinates, c + 1 = (c - 1) + 2; bit o of
// `inside` is set where corner o has f < 0, and a cell with none or all of them inside holds no triangle.
template <typename F>
__device__ __forceinline__ void for_each_crossed_cell(const unsigned (&w)[kWordsPerThread], const Lattice& L, F f) {
  const int64_t cside = L.side - 1;
  const int64_t word0 = (int64_t)blockIdx.x * kScanWords + (int64_t)threadIdx.x * kWordsPerThread;
  for (int k = 0; k < kWordsPerThread; ++k) {
    unsigned x = w[k];
    while (x) {
      const int b = __ffs(x) - 1;
      x &= x - 1;
      const int64_t key = (word0 + k) * 32 + b;
      const int cx = (int)(key / (cside * cside)), cy = (int)(key / cside % cside), cz = (int)(key % cside);
      unsigned inside = 0;
#pragma unroll
      for (int o = 0; o < 8; ++o)
        if (f_at(L, cx + (o >> 2), cy + ((o >> 1) & 1), cz + (o & 1)) < 0.0) inside |= 1u << o;
      if (inside == 0u || inside == 255u) continue;
      f(cx, cy, cz, inside);
    }
  }
}

// EMIT = false: block_tri[b] = the triangles of scan block b.  EMIT = true: block_tri holds the exclusive prefix and the
// triangles are written, three edge ids each, in the order of the cells' keys.
template <bool EMIT>
__global__ void __launch_bounds__(kScanThreads) surface_triangles_kernel(const unsigned* cbits, Lattice L, int64_t* block_tri,
                                                                         int64_t n_triangles, int64_t* tri_ids) {
  unsigned w[kWordsPerThread];
  const unsigned any = load_words(cbits, blockIdx.x, w);
  unsigned count = 0;
  if (any)
    for_each_crossed_cell(w, L, [&](int, int, int, unsigned inside) { cell_triangles(inside, [&](int, int, int) { ++count; }); });
  unsigned total;
  const unsigned before = block_scan(count, &total);
  if (!EMIT) {
    if (threadIdx.x == 0) block_tri[blockIdx.x] = total;
    return;
  }
  if (count == 0) return;
  int64_t o = block_tri[blockIdx.x] + before;
  for_each_crossed_cell(w, L, [&](int cx, int cy, int cz, unsigned inside) {
    auto id = [&](int e) {
      const int lo = e >> 3, hi = e & 7;
      return cell_of(L.side, cx + (lo >> 2), cy + ((lo >> 1) & 1), cz + (lo & 1)) * 7 + direction_of(hi ^ lo);
    };
    cell_triangles(inside, [&](int e0, int e1, int e2) {
      if (o < n_triangles) {
        tri_ids[o * 3] = id(e0);
        tri_ids[o * 3 + 1] = id(e1);
        tri_ids[o * 3 + 2] = id(e2);
      }
      ++o;
    });
  });
}

// the mesh vertex on lattice edge id = key(a) * 7 + direction
__global__ void __launch_bounds__(kSurfThreads) surface_vertices_kernel(const int64_t* ids, int64_t n_ids, Lattice L, double* vertices) {
  const int64_t v = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (v >= n_ids) return;
  const int64_t id = ids[v], key = id / 7, side = L.side;
  const int dir = (int)(id % 7);
  const int db = direction_bits(dir);
  const int d[3] = {(db >> 2) & 1, (db >> 1) & 1, db & 1};
  const int a[3] = {(int)(key / (side * side)), (int)(key / side % side), (int)(key % side)};
  const double fa = f_at(L, a[0], a[1], a[2]), fb = f_at(L, a[0] + d[0], a[1] + d[1], a[2] + d[2]);
  const double t = fa / (fa - fb);
#pragma unroll
  for (int c = 0; c < 3; ++c) vertices[v * 3 + c] = ((double)(a[c] - 2) + 0.5) + t * (double)d[c];
}

__global__ void __launch_bounds__(kSurfThreads) surface_index_kernel(const int64_t* ids, int64_t n_ids, const int64_t* tri_ids, int64_t n,
                                                                    int32_t* triangles) {
  const int64_t j = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
  if (j >= n) return;
  triangles[j] = (int32_t)find_sorted_key(ids, n_ids, tri_ids[j]);
}

bool surface_size_ok(int bits, int64_t n) { return bits >= 1 && bits <= kSurfMaxBits && n >= 1 && n <= 0x7FFFFFFF; }

// the occupancy rank structure, then
struct SurfaceBuffers {
  RankBuffers occ;
  unsigned* order;            // [n] rank -> row
  int8_t* sign[2];            // [n] each, by rank
  OrientState* state;
  unsigned* cbits;            // candidate cells over (res + 2)^3
  int64_t *cblock, *tblock;   // per scan block of cbits: cells before it, triangles before it
  int64_t *n_cells, *n_triangles;
  RankBuffers ver;            // lattice vertices over (res + 3)^3
  double* normals;            // [n, 3] oriented, by rank
  int64_t cblk, vblk;         // scan blocks of cbits and of ver.bits
  size_t bytes;
};

SurfaceBuffers surface_layout(int bits, int64_t n, void* workspace) {
  const int res = 1 << bits;
  SurfaceBuffers b;
  b.cblk = scan_blocks((int64_t)(res + 2) * (res + 2) * (res + 2));
  b.vblk = scan_blocks((int64_t)(res + 3) * (res + 3) * (res + 3));
  b.occ = rank_layout(res, workspace);
  Carver& c = b.occ.rest;
  b.order = c.take<unsigned>((size_t)n);
  for (int k = 0; k < 2; ++k) b.sign[k] = c.take<int8_t>((size_t)n);
  b.state = c.take<OrientState>(1);
  b.cbits = c.take<unsigned>(padded_bits_words(b.cblk));
  b.cblock = c.take<int64_t>((size_t)b.cblk);
  b.tblock = c.take<int64_t>((size_t)b.cblk);
  b.n_cells = c.take<int64_t>(2);
  b.n_triangles = b.n_cells + 1;
  b.ver = rank_layout(res + 3, c);
  b.normals = b.ver.rest.take<double>((size_t)n * 3);
  b.bytes = b.ver.rest.bytes();
  return b;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kSurfThreads - 1) / kSurfThreads); }

// the occupancy bit set, its rank table and the rows in key order
int surface_prepare(const SurfaceBuffers& b, const int32_t* points, int64_t n, int res, hipStream_t s) {
  if (int rc = build_rank(b.occ, res, points, nullptr, n, s)) return rc;
  hipLaunchKernelGGL(surface_order_kernel, dim3(blocks_for(n)), dim3(kSurfThreads), 0, s, points, n, res, b.occ.bits, b.occ.rank, b.order);
  return 0;
}

Lattice lattice_of(const SurfaceBuffers& b, int res, const double* f, int64_t n_vertices) {
  Lattice L;
  L.vbits = b.ver.bits;
  L.vrank = b.ver.rank;
  L.f = f;
  L.n_vertices = n_vertices;
  L.side = res + 3;
  return L;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_surface_workspace_bytes(int bits, int64_t n) { return surface_size_ok(bits, n) ? surface_layout(bits, n, nullptr).bytes : 0; }

int pcgc_surface_orient(const int32_t* points, const float* normals, const uint8_t* seed, int64_t n, int bits, int gap, const double* tau,
                        int n_tau, int batch, int8_t* sign, int32_t* rounds, int32_t* readbacks, void* workspace, size_t workspace_bytes,
                        pcgc_stream_t stream) {
  PCGC_REQUIRE(points && normals && seed && tau && sign && rounds && workspace && surface_size_ok(bits, n),
               "pcgc_surface_orient: bad arguments");
  PCGC_REQUIRE(gap >= 1 && gap <= kSurfMaxGap, "pcgc_surface_orient: gap = %d outside 1..%d", gap, kSurfMaxGap);
  PCGC_REQUIRE(n_tau >= 1 && n_tau <= kSurfMaxStages, "pcgc_surface_orient: %d stage thresholds, 1..%d are allowed", n_tau, kSurfMaxStages);
  for (int k = 0; k < n_tau; ++k)
    PCGC_REQUIRE(tau[k] >= 0.0 && tau[k] <= 1.0, "pcgc_surface_orient: stage threshold %d = %g outside [0, 1]", k, tau[k]);
  PCGC_REQUIRE(tau[n_tau - 1] == 0.0, "pcgc_surface_orient: the last stage threshold is %g, it must be 0.0", tau[n_tau - 1]);
  PCGC_REQUIRE(batch >= 1 && batch <= 4096, "pcgc_surface_orient: batch = %d outside 1..4096", batch);
  hipStream_t s = (hipStream_t)stream;
  const int res = 1 << bits;
  const SurfaceBuffers b = surface_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_surface_orient: workspace too small");
  Tau t;
  t.n = n_tau;
  for (int k = 0; k < kSurfMaxStages; ++k) t.v[k] = k < n_tau ? tau[k] : 0.0;
  if (int rc = surface_prepare(b, points, n, res, s)) return rc;
  PCGC_CHECK_HIP(hipMemsetAsync(b.state, 0, sizeof(OrientState), s));
  hipLaunchKernelGGL(surface_seed_kernel, dim3(blocks_for(n)), dim3(kSurfThreads), 0, s, normals, seed, b.order, b.occ.n_set, b.sign[0],
                     b.state);
  hipLaunchKernelGGL(surface_tail_kernel, dim3(1), dim3(1), 0, s, b.state, n_tau, 0);
  // Round t reads sign[t & 1] and writes the other buffer; a round launched after the end returns at once and writes nothing,
  // so the result is in sign[rounds & 1].  One read-back of the state per batch.
  OrientState st;
  int launched = 0, reads = 0;
  for (;;) {
    PCGC_CHECK_HIP(hipMemcpyAsync(&st, b.state, sizeof(st), hipMemcpyDeviceToHost, s));
    PCGC_CHECK_HIP(hipStreamSynchronize(s));
    ++reads;
    if (st.done) break;
    for (int k = 0; k < batch; ++k, ++launched) {
      hipLaunchKernelGGL(surface_round_kernel, dim3(blocks_for(n)), dim3(kSurfThreads), 0, s, points, normals, b.order, b.occ.n_set, bits, gap,
                         b.occ.bits, b.occ.rank, t, b.sign[launched & 1], b.sign[(launched + 1) & 1], b.state);
      hipLaunchKernelGGL(surface_tail_kernel, dim3(1), dim3(1), 0, s, b.state, n_tau, 1);
    }
  }
  if (int rc = launch_ok("orientation kernels")) return rc;
  PCGC_REQUIRE(st.done == 1, "pcgc_surface_orient: a component holds no seed, its voxels cannot be set");
  hipLaunchKernelGGL(surface_sign_gather_kernel, dim3(blocks_for(n)), dim3(kSurfThreads), 0, s, points, n, res, b.occ.bits, b.occ.rank,
                     b.sign[st.rounds & 1], sign);
  *rounds = st.rounds;
  if (readbacks) *readbacks = reads;
  return launch_ok("orientation kernels");
}

int pcgc_surface_lattice(const int32_t* points, int64_t n, int bits, int64_t* counts, void* workspace, size_t workspace_bytes,
                         pcgc_stream_t stream) {
  PCGC_REQUIRE(points && counts && workspace && surface_size_ok(bits, n), "pcgc_surface_lattice: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int res = 1 << bits;
  const SurfaceBuffers b = surface_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_surface_lattice: workspace too small");
  if (int rc = surface_prepare(b, points, n, res, s)) return rc;
  PCGC_CHECK_HIP(hipMemsetAsync(b.cbits, 0, padded_bits_bytes(b.cblk), s));
  PCGC_CHECK_HIP(hipMemsetAsync(b.ver.bits, 0, padded_bits_bytes(b.vblk), s));
  hipLaunchKernelGGL(surface_mark_kernel, dim3(blocks_for(n)), dim3(kSurfThreads), 0, s, points, n, res, b.cbits, b.ver.bits);
  hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)b.cblk), dim3(kScanThreads), 0, s, b.cbits, b.cblock);
  hipLaunchKernelGGL(grid_block_scan_kernel, dim3(1), dim3(1024), 0, s, b.cblock, b.cblk, b.n_cells);
  hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)b.vblk), dim3(kScanThreads), 0, s, b.ver.bits, b.ver.block_count);
  hipLaunchKernelGGL(grid_block_scan_kernel, dim3(1), dim3(1024), 0, s, b.ver.block_count, b.vblk, b.ver.n_set);
  hipLaunchKernelGGL(rank_write_kernel, dim3((unsigned)b.vblk), dim3(kScanThreads), 0, s, b.ver.bits, b.ver.block_count, b.ver.rank);
  hipLaunchKernelGGL(surface_counts_kernel, dim3(1), dim3(1), 0, s, b.n_cells, b.ver.n_set, counts);
  return launch_ok("lattice kernels");
}

int pcgc_surface_implicit(const double* oriented_normals, int64_t n, int bits, int radius, int64_t n_vertices, int64_t* vertex_keys, double* f,
                          void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(oriented_normals && vertex_keys && f && workspace && surface_size_ok(bits, n) && n_vertices >= 1,
               "pcgc_surface_implicit: bad arguments");
  PCGC_REQUIRE(radius >= kSurfMinRadius && radius <= kSurfMaxRadius, "pcgc_surface_implicit: radius = %d outside %d..%d", radius,
               kSurfMinRadius, kSurfMaxRadius);
  hipStream_t s = (hipStream_t)stream;
  const int res = 1 << bits;
  const SurfaceBuffers b = surface_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_surface_implicit: workspace too small");
  hipLaunchKernelGGL(surface_vertex_list_kernel, dim3((unsigned)b.vblk), dim3(kScanThreads), 0, s, b.ver.bits, b.ver.block_count, n_vertices,
                     vertex_keys);
  hipLaunchKernelGGL(surface_normals_kernel, dim3(blocks_for(n)), dim3(kSurfThreads), 0, s, oriented_normals, b.order, b.occ.n_set, b.normals);
  hipLaunchKernelGGL(surface_implicit_kernel, dim3(blocks_for(n_vertices)), dim3(kSurfThreads), 0, s, vertex_keys, n_vertices, b.ver.n_set, res,
                     radius, b.occ.bits, b.occ.rank, b.normals, f);
  return launch_ok("implicit kernels");
}

int pcgc_surface_triangles(const double* f, int64_t n_vertices, int64_t n, int bits, int64_t n_triangles, int64_t* triangle_ids,
                           int64_t* count, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(f && workspace && surface_size_ok(bits, n) && n_vertices >= 1 && n_triangles >= 0, "pcgc_surface_triangles: bad arguments");
  PCGC_REQUIRE((triangle_ids != nullptr) != (count != nullptr), "pcgc_surface_triangles: give count (first call) or triangle_ids (second)");
  hipStream_t s = (hipStream_t)stream;
  const int res = 1 << bits;
  const SurfaceBuffers b = surface_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_surface_triangles: workspace too small");
  const Lattice L = lattice_of(b, res, f, n_vertices);
  if (count) {
    hipLaunchKernelGGL(surface_triangles_kernel<false>, dim3((unsigned)b.cblk), dim3(kScanThreads), 0, s, b.cbits, L, b.tblock, (int64_t)0,
                       (int64_t*)nullptr);
    hipLaunchKernelGGL(grid_block_scan_kernel, dim3(1), dim3(1024), 0, s, b.tblock, b.cblk, b.n_triangles);
    PCGC_CHECK_HIP(hipMemcpyAsync(count, b.n_triangles, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  } else if (n_triangles > 0) {
    hipLaunchKernelGGL(surface_triangles_kernel<true>, dim3((unsigned)b.cblk), dim3(kScanThreads), 0, s, b.cbits, L, b.tblock, n_triangles,
                       triangle_ids);
  }
  return launch_ok("triangle kernels");
}

int pcgc_surface_mesh(const int64_t* edge_ids, int64_t n_edges, const int64_t* triangle_ids, int64_t n_triangles, const double* f,
                      int64_t n_vertices, int64_t n, int bits, double* vertices, int32_t* triangles, void* workspace, size_t workspace_bytes,
                      pcgc_stream_t stream) {
  PCGC_REQUIRE(edge_ids && triangle_ids && f && vertices && triangles && workspace && surface_size_ok(bits, n) && n_vertices >= 1 &&
                   n_edges >= 1 && n_edges <= 0x7FFFFFFF && n_triangles >= 1,
               "pcgc_surface_mesh: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const SurfaceBuffers b = surface_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_surface_mesh: workspace too small");
  const Lattice L = lattice_of(b, 1 << bits, f, n_vertices);
  hipLaunchKernelGGL(surface_vertices_kernel, dim3(blocks_for(n_edges)), dim3(kSurfThreads), 0, s, edge_ids, n_edges, L, vertices);
  hipLaunchKernelGGL(surface_index_kernel, dim3(blocks_for(n_triangles * 3)), dim3(kSurfThreads), 0, s, edge_ids, n_edges, triangle_ids,
                     n_triangles * 3, triangles);
  return launch_ok("mesh kernels");
}

}  // extern "C"
