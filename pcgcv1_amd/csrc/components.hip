// Connected components of a voxel cloud (gfx950): what pcgcv1_amd/clean.py drops islands of a raw scan on.
//
// include/pcgc.h states the rule (tests/_components_ref.py restates it in numpy).  Two voxels are linked when
// their Chebyshev distance is at most the gap G; label = the smallest key of a voxel's component, size = its voxel count.
//
// The cloud is voxel_grid.h's bit set with its rank table, so an occupied cell's rank (its index among the set bits in key
// order) is two loads and the smallest rank of a component is its smallest key.  parent[r] is a union-find forest over the
// ranks with parent[r] <= r from the first store on:
//   * components_list_kernel    key[r] of every set bit, parent[r] = r, count[r] = 0;
//   * components_hook_kernel    a voxel looks at the cells of its (2G+1)^3 window that have a smaller key (the columns before
//     its own in full, its own column below it; the following half is the other voxel's preceding half), z-runs read as one
//     or two masked words the way clean_neighbors_kernel reads its columns, and unites itself with every occupied one: both
//     roots are found, the larger is hooked under the smaller by a compare-and-swap on its own parent word.  Only a root is
//     ever hooked and only under a smaller rank, so the root of a finished tree is its smallest rank whatever the order of
//     the threads;
//   * components_flatten_kernel (a launch of its own) parent[r] = root(r), count[root] += 1, the roots counted;
//   * components_gather_kernel  per input row: rank of its cell -> root -> key[root], count[root].
// No thread waits for another: the only retry is a compare-and-swap that failed because some other thread hooked that root,
// after which this thread goes on from the smaller rank it was handed.  Every chain walk follows strictly decreasing ranks
// and so ends on any contents of parent.  In the hook kernel parent is read by agent-scope relaxed atomic loads and written
// by agent-scope atomics only: a CU's L1 and the other XCDs' L2 are not refreshed by a store, and a stale parent costs a
// failed compare-and-swap, never a wrong link.  Integer atomics throughout: two runs give the same bytes.
#include <algorithm>
#include "common.h"
#include "voxel_grid.h"

namespace pcgc {
namespace {

constexpr int kCompMaxBits = 12, kCompMaxGap = 8;
constexpr int kHookThreads = 256;
constexpr int kFlattenThreads = 1024, kFlattenWaves = kFlattenThreads / 64;

__device__ __forceinline__ unsigned load_parent(const unsigned* parent, unsigned x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree.  A step needs parent < x, so the walk ends after at most x steps whatever parent holds.  On the way
// x is pointed at its grandparent (path halving): an ancestor stays an ancestor, and the minimum keeps parent[x] <= x.
__device__ __forceinline__ unsigned find_root(unsigned* parent, unsigned x) {
  unsigned p = load_parent(parent, x);
  while (p < x) {
    const unsigned g = load_parent(parent, p);
    if (g < p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// One tree out of a's and b's -> its root as this thread last saw it.  The compare-and-swap succeeds only while the larger
// root is still a root; when it fails, `seen` is the smaller rank somebody else hooked it under.
__device__ __forceinline__ unsigned unite(unsigned* parent, unsigned a, unsigned b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return a;
    if (a < b) { const unsigned t = a; a = b; b = t; }
    unsigned seen = a;
    if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return b;
    a = seen;
  }
}

__global__ void __launch_bounds__(kScanThreads) components_list_kernel(const unsigned* bits, const int64_t* block_offset, int64_t* key,
                                                                       unsigned* parent, unsigned* count, unsigned* n_roots) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_roots = 0;
  for_each_set_bit(bits, block_offset, [&](int64_t o, int64_t k) {
    key[o] = k;
    parent[o] = (unsigned)o;
    count[o] = 0;
  });
}

// L lanes share a voxel and take every L-th column (dx, dy) of the preceding half window, in key order: column c is
// (c / side - G, c % side - G) for c = 0 .. G * side + G, the last one the voxel's own, of which only the cells below it
// count.  The lanes of a voxel do not talk to each other: each unites what it finds, starting from the root it reached last.
template <int L>
__global__ void __launch_bounds__(kHookThreads) components_hook_kernel(const int64_t* key, const int64_t* n_set, int bits_per_axis, int G,
                                                                       const unsigned* bits, const unsigned* rank, unsigned* parent) {
  const int64_t t = (int64_t)blockIdx.x * kHookThreads + threadIdx.x;
  const int64_t r = t / L;
  if (r >= *n_set) return;
  const int res = 1 << bits_per_axis;
  const int64_t k = key[r];
  const int x = (int)(k >> (2 * bits_per_axis)), y = (int)(k >> bits_per_axis) & (res - 1), z = (int)k & (res - 1);
  const int side = 2 * G + 1, own = G * side + G;
  unsigned root = (unsigned)r;
  for (int c = (int)(t % L); c <= own; c += L) {
    const int cx = c / side;
    const int qx = x + cx - G, qy = y + c - cx * side - G;
    if ((unsigned)qx >= (unsigned)res || (unsigned)qy >= (unsigned)res) continue;
    const int z0 = max(z - G, 0), z1 = c == own ? z - 1 : min(z + G, res - 1);        // the z-run, inside the row
    if (z1 < z0) continue;
    const int64_t row = cell_of(res, qx, qy, 0);
    for_each_in_run(bits, row + z0, row + z1, [&](int64_t w, unsigned all, int b) {
      root = unite(parent, root, rank[w] + __popc(all & ((1u << b) - 1u)));            // rank_of the cell w * 32 + b
    });
  }
}

// parent[r] = root(r) for every rank, count[root] += 1 and *n_roots += 1 per root.  The adds are combined first: the lanes of
// a wave that found the same root add once, and the first such group of every wave goes through LDS so that a workgroup
// whose waves agree (ranks that follow each other mostly share a component) adds once; one word would otherwise take an add
// per voxel of the largest component.  No wave leaves before the barrier.
__global__ void __launch_bounds__(kFlattenThreads) components_flatten_kernel(const int64_t* n_set, unsigned* parent, unsigned* count,
                                                                             unsigned* n_roots) {
  __shared__ unsigned wave_root[kFlattenWaves], wave_count[kFlattenWaves], wave_roots[kFlattenWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * kFlattenThreads + threadIdx.x;
  const bool live = r < *n_set;
  unsigned root = 0;
  if (live) {
    root = find_root(parent, (unsigned)r);
    __hip_atomic_store(parent + r, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  unsigned long long todo = __ballot(live);
  const unsigned long long roots = __ballot(live && root == (unsigned)r);
  if (lane == 0) { wave_count[wave] = 0; wave_roots[wave] = (unsigned)__popcll(roots); }
  for (bool first = true; todo; first = false) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned lr = __shfl(root, leader);
    const unsigned long long same = __ballot(live && root == lr) & todo;
    if (lane == leader) {
      if (first) { wave_root[wave] = lr; wave_count[wave] = (unsigned)__popcll(same); }
      else atomicAdd(&count[lr], (unsigned)__popcll(same));
    }
    todo &= ~same;
  }
  __syncthreads();
  if (threadIdx.x < kFlattenWaves && wave_count[threadIdx.x]) {      // the first wave holding a root adds for all that hold it
    const unsigned mine = wave_root[threadIdx.x];
    unsigned total = 0;
    bool earlier = false;
    for (int v = 0; v < kFlattenWaves; ++v)
      if (wave_count[v] && wave_root[v] == mine) {
        earlier |= v < (int)threadIdx.x;
        total += wave_count[v];
      }
    if (!earlier) atomicAdd(&count[mine], total);
  }
  if (threadIdx.x == 0) {
    unsigned total = 0;
    for (int v = 0; v < kFlattenWaves; ++v) total += wave_roots[v];
    if (total) atomicAdd(n_roots, total);
  }
}

// label and size (or NULL) of input row i; a row outside the grid set no bit and belongs to no component
__global__ void __launch_bounds__(256) components_gather_kernel(const int32_t* p, int64_t n, int res, const unsigned* bits, const unsigned* rank,
                                                                const unsigned* parent, const unsigned* count, const int64_t* key,
                                                                const unsigned* n_roots, int64_t* label, int32_t* size,
                                                                int64_t* n_components) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0 && n_components) *n_components = (int64_t)*n_roots;
  if (i >= n) return;
  const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
  int64_t l = -1;
  int32_t s = 0;
  if (in_grid(res, x, y, z)) {
    const unsigned root = parent[rank_of(bits, rank, cell_of(res, x, y, z))];
    l = key[root];
    s = (int32_t)count[root];
  }
  label[i] = l;
  if (size) size[i] = s;
}

bool components_size_ok(int bits, int64_t n) { return bits >= 1 && bits <= kCompMaxBits && n >= 1 && n <= 0x7FFFFFFF; }

// the rank structure, then key [n] int64, parent [n], count [n], the number of roots
struct ComponentBuffers { RankBuffers r; int64_t* key; unsigned *parent, *count, *n_roots; size_t bytes; };

ComponentBuffers components_layout(int bits, int64_t n, void* workspace) {
  ComponentBuffers c;
  c.r = rank_layout(1 << bits, workspace);
  Carver& rest = c.r.rest;
  c.key = rest.take<int64_t>((size_t)n);
  c.parent = rest.take<unsigned>((size_t)n);
  c.count = rest.take<unsigned>((size_t)n);
  c.n_roots = rest.take<unsigned>(1);
  c.bytes = rest.bytes();
  return c;
}

template <int L>
void launch_hook(int64_t n, const ComponentBuffers& c, int bits, int gap, hipStream_t s) {
  hipLaunchKernelGGL(components_hook_kernel<L>, dim3((unsigned)((n * L + kHookThreads - 1) / kHookThreads)), dim3(kHookThreads), 0, s, c.key,
                     c.r.n_set, bits, gap, c.r.bits, c.r.rank, c.parent);
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_clean_components_workspace_bytes(int bits, int64_t n) {
  return components_size_ok(bits, n) ? components_layout(bits, n, nullptr).bytes : 0;
}

int pcgc_clean_components(const int32_t* points, int64_t n, int bits, int gap, int64_t* label, int32_t* size, int64_t* n_components,
                          void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && label && workspace && components_size_ok(bits, n), "pcgc_clean_components: bad arguments");
  PCGC_REQUIRE(gap >= 1 && gap <= kCompMaxGap, "pcgc_clean_components: gap = %d outside 1..%d", gap, kCompMaxGap);
  const ComponentBuffers c = components_layout(bits, n, workspace);
  PCGC_REQUIRE(workspace_bytes >= c.bytes, "pcgc_clean_components: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int res = 1 << bits;
  const RankBuffers& r = c.r;
  const int64_t nblk = scan_blocks((int64_t)res * res * res);
  if (int rc = build_rank(r, res, points, nullptr, n, s)) return rc;
  hipLaunchKernelGGL(components_list_kernel, dim3((unsigned)nblk), dim3(kScanThreads), 0, s, r.bits, r.block_count, c.key, c.parent, c.count,
                     c.n_roots);
  // Lanes per voxel, as measured: a lane that walks its columns one after the other carries the root it has
  // reached from one neighbour to the next, so few lanes beat many; one lane up to the 25 columns of G = 3, two from the 41
  // of G = 4 to the 145 of G = 8.  The grids are sized for n, an upper bound of the set bits, which the kernels read on the
  // device.
  if (gap <= 3) launch_hook<1>(n, c, bits, gap, s);
  else launch_hook<2>(n, c, bits, gap, s);
  hipLaunchKernelGGL(components_flatten_kernel, dim3((unsigned)((n + kFlattenThreads - 1) / kFlattenThreads)), dim3(kFlattenThreads), 0, s,
                     r.n_set, c.parent, c.count, c.n_roots);
  hipLaunchKernelGGL(components_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, n, res, r.bits, r.rank, c.parent,
                     c.count, c.key, c.n_roots, label, size, n_components);
  return launch_ok("component kernels");
}

}  // extern "C"
