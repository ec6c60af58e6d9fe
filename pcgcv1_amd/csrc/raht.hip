// RAHT colour transform (gfx950): the region-adaptive hierarchical transform over the Morton order of a voxelised cloud, its
// quantiser and the symbol preparation of the colour codec (pcgcv1_amd/colorcodec.py).  DESIGN.md §7d states the rule;
// tests/_raht_ref.py is its definition in numpy.
//
// The tree is never materialised level by level.  With the keys sorted, leaf j > 0 differs from leaf j - 1 first (from the
// top) at bit h[j] = 63 - clz(key[j] ^ key[j-1]).  At level l the nodes are the runs of equal key >> l, and a run is named
// by its first leaf.  The node that starts at leaf j exists at levels 0 .. h[j] and is the RIGHT sibling of exactly one merge, at
// level h[j]; its left sibling starts at the first leaf of the run of key >> (h[j] + 1), found by a binary search in the sorted
// keys, as is the end of its own run.  So one pass over the leaves yields per leaf: the level of its merge (its subband), the
// slot of its left sibling and both weights (j - left, right_end - j).  The transform then runs IN PLACE on one [M,3] float64
// array: the merge of leaf j reads slots left[j] and j, writes the low-pass value to left[j] and the coefficient to j; slot 0
// ends as the DC.  The merges of one level touch disjoint slots (a node has one sibling), so no atomics are needed and the
// levels are the only dependence.  The leaves grouped by level (a stable counting sort: per-block histograms, a
// one-workgroup scan, a write pass) give each level's work list and the subband order of the symbols.
//
// Every output is defined bit for bit: float64 sqrt and division are correctly rounded, the file is built with
// -ffp-contract=off, no step adds more than two terms, and everything else is integer arithmetic.
#include <algorithm>
#include "common.h"
#include "workspace.h"

namespace pcgc {
namespace {

constexpr int kMaxDepth = 12;                    // 36-bit keys, 36 levels
constexpr int kBins = 3 * kMaxDepth + 1;         // subbands 0 .. 3d-1 and the DC (3d)
constexpr int kThreads = 256;
constexpr int kScanSegs = 16;                    // the block-histogram scan: kScanSegs segments of blocks x kBins bins
constexpr int kTop = 1024;                       // merges (the DC's entry included) that the one-workgroup tree top holds

__device__ __forceinline__ int64_t spread3(int v) {            // bit b of v -> bit 3b
  int64_t x = (int64_t)(v & 0xFFF);
  x = (x | (x << 16)) & 0x0000FF0000FFll;
  x = (x | (x << 8)) & 0x00F00F00F00Fll;
  x = (x | (x << 4)) & 0x0C30C30C30C3ll;
  x = (x | (x << 2)) & 0x249249249249ll;
  return x;
}

__global__ void __launch_bounds__(kThreads) keys_kernel(const int32_t* p, int64_t m, int64_t* keys) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  keys[i] = (spread3(p[i * 3]) << 2) | (spread3(p[i * 3 + 1]) << 1) | spread3(p[i * 3 + 2]);
}

// first index in [lo, hi) whose key is >= v (hi if none)
__device__ __forceinline__ int64_t lower_bound(const int64_t* keys, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// per leaf: subband, left sibling's slot, right weight; per block: the histogram of the subbands
__global__ void __launch_bounds__(kThreads) structure_kernel(const int64_t* keys, int64_t m, int nlev, int32_t* subband, int32_t* left,
                                                             int32_t* w_right, int32_t* block_hist, int32_t* bad) {
  __shared__ int hist[kBins];
  if (threadIdx.x < kBins) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j < m) {
    int h = nlev;
    int64_t l = 0, r = m;
    if (j > 0) {
      const int64_t k = keys[j], x = k ^ keys[j - 1];
      if (x <= 0 || k < keys[j - 1] || (k >> nlev) != 0) {          // duplicate, unsorted or out of range: refuse, touch nothing else
        atomicOr(bad, 1);
        h = 0; l = j - 1; r = j + 1;
      } else {
        h = 63 - __clzll(x);
        l = lower_bound(keys, 0, j, (k >> (h + 1)) << (h + 1));
        r = lower_bound(keys, j + 1, m, ((k >> h) + 1) << h);
      }
    } else if (keys[0] < 0 || (keys[0] >> nlev) != 0) {
      atomicOr(bad, 1);
    }
    subband[j] = h;
    left[j] = (int32_t)l;
    w_right[j] = (int32_t)(r - j);
    atomicAdd(&hist[h], 1);
  }
  __syncthreads();
  if (threadIdx.x < kBins) block_hist[(int64_t)blockIdx.x * kBins + threadIdx.x] = hist[threadIdx.x];
}

// block_hist[blk][b] becomes the position in `order` of block blk's first leaf of subband b; level_counts[b] = leaves of subband b
__global__ void __launch_bounds__(kScanSegs * 64) hist_scan_kernel(int32_t* block_hist, int64_t nblk, int64_t* level_counts) {
  __shared__ int64_t part[kScanSegs][64];
  const int b = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int64_t per = (nblk + kScanSegs - 1) / kScanSegs;
  const int64_t b0 = std::min<int64_t>(nblk, seg * per), b1 = std::min<int64_t>(nblk, b0 + per);
  int64_t s = 0;
  if (b < kBins)
    for (int64_t k = b0; k < b1; ++k) s += block_hist[k * kBins + b];
  part[seg][b] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc = 0;
    for (int bb = 0; bb < kBins; ++bb) {
      int64_t total = 0;
      for (int sg = 0; sg < kScanSegs; ++sg) { const int64_t x = part[sg][bb]; part[sg][bb] = acc + total; total += x; }
      level_counts[bb] = total;
      acc += total;
    }
  }
  __syncthreads();
  if (b < kBins) {
    int64_t acc = part[seg][b];
    for (int64_t k = b0; k < b1; ++k) { const int x = block_hist[k * kBins + b]; block_hist[k * kBins + b] = (int32_t)acc; acc += x; }
  }
}

// order[position] = leaf, subbands ascending, leaves ascending within a subband
__global__ void __launch_bounds__(kThreads) order_kernel(const int32_t* subband, int64_t m, int nbins, const int32_t* block_off,
                                                         int32_t* order) {
  __shared__ int wcount[kThreads / 64][kBins];
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = j < m ? subband[j] : -1;
  int r = 0;
  for (int b = 0; b < nbins; ++b) {
    const unsigned long long mask = __ballot(h == b);
    if (lane == 0) wcount[wave][b] = __popcll(mask);
    if (h == b) r = __popcll(mask & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (h < 0) return;
  int base = block_off[(int64_t)blockIdx.x * kBins + h];
  for (int w = 0; w < wave; ++w) base += wcount[w][h];
  order[base + r] = (int32_t)j;
}

// ---------------------------------------------------------------------------------------------------------------- the butterflies
// tests/_raht_ref.py, step 3: this expression order
__device__ __forceinline__ void forward_pair(double s1, double s2, double sw, const double* a1, const double* a2, double* lo, double* hi) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = (s1 * a1[c] + s2 * a2[c]) / sw;
    hi[c] = (s1 * a2[c] - s2 * a1[c]) / sw;
  }
}

// step 5
__device__ __forceinline__ void inverse_pair(double s1, double s2, double sw, const double* lo, const double* hi, double* a1, double* a2) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a1[c] = (s1 * lo[c] - s2 * hi[c]) / sw;
    a2[c] = (s2 * lo[c] + s1 * hi[c]) / sw;
  }
}

// one lane per merge of one level: the leaves order[k0 .. k0 + n)
template <bool kInverse>
__global__ void __launch_bounds__(kThreads) level_kernel(double* attr, const int32_t* order, int64_t k0, int64_t n, const int32_t* left,
                                                         const int32_t* w_right) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= n) return;
  const int64_t j = order[k0 + t], p = left[j];
  const double w1 = (double)(j - p), w2 = (double)w_right[j];
  const double s1 = sqrt(w1), s2 = sqrt(w2), sw = sqrt(w1 + w2);
  double x[3], y[3], u[3], v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { x[c] = attr[p * 3 + c]; y[c] = attr[j * 3 + c]; }
  if (kInverse) inverse_pair(s1, s2, sw, x, y, u, v); else forward_pair(s1, s2, sw, x, y, u, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) { attr[p * 3 + c] = u[c]; attr[j * 3 + c] = v[c]; }
}

// every level from l0 up in one workgroup: the n <= kTop leaves order[k0 .. k0 + n) (the last one is leaf 0, the DC's slot) live
// in LDS, thread t owns leaf order[k0 + t]; pos[leaf] = its thread (written here, read only at leaves of this list)
template <bool kInverse>
__global__ void __launch_bounds__(kTop) top_kernel(double* attr, const int32_t* order, int64_t k0, int n, const int32_t* left,
                                                   const int32_t* w_right, const int32_t* subband, int32_t* pos, int l0, int nlev) {
  __shared__ double s[kTop][3];
  const int t = threadIdx.x;
  const bool active = t < n;
  int64_t j = 0;
  if (active) {
    j = order[k0 + t];
    pos[j] = t;
  }
  __syncthreads();
  int h = -1, p = 0;
  double s1 = 0.0, s2 = 0.0, sw = 1.0;
  if (active) {
    h = subband[j];
    const int64_t lj = left[j];
    p = h < nlev ? min(max(pos[lj], 0), kTop - 1) : t;          // pos[lj] was written above: lj's own merge is at a higher level
    const double w1 = (double)(j - lj), w2 = (double)w_right[j];
    s1 = sqrt(w1); s2 = sqrt(w2); sw = sqrt(w1 + w2);
#pragma unroll
    for (int c = 0; c < 3; ++c) s[t][c] = attr[j * 3 + c];
  }
  __syncthreads();
  for (int i = 0; i < nlev - l0; ++i) {
    const int l = kInverse ? nlev - 1 - i : l0 + i;
    if (h == l) {
      double x[3], y[3], u[3], v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { x[c] = s[p][c]; y[c] = s[t][c]; }
      if (kInverse) inverse_pair(s1, s2, sw, x, y, u, v); else forward_pair(s1, s2, sw, x, y, u, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) { s[p][c] = u[c]; s[t][c] = v[c]; }
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (int c = 0; c < 3; ++c) attr[j * 3 + c] = s[t][c];
  }
}

// ---------------------------------------------------------------------------------------------------------------- colours in and out
// YCoCg-R of point point_of_leaf[j] into slot j (step 1)
__global__ void __launch_bounds__(kThreads) load_colors_kernel(const uint8_t* rgb, const int64_t* point_of_leaf, int64_t m, double* attr) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const int64_t i = point_of_leaf[j];
  const int r = rgb[i * 3], g = rgb[i * 3 + 1], b = rgb[i * 3 + 2];
  const int co = r - b, t = b + (co >> 1), cg = g - t, y = t + (cg >> 1);
  attr[j * 3] = (double)y; attr[j * 3 + 1] = (double)co; attr[j * 3 + 2] = (double)cg;
}

// step 6: rint, clip to the channel's range, inverse YCoCg-R, clip to [0, 255]
__global__ void __launch_bounds__(kThreads) store_colors_kernel(const double* attr, const int64_t* point_of_leaf, int64_t m, uint8_t* rgb) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const int64_t i = point_of_leaf[j];
  const int y = (int)fmin(fmax(rint(attr[j * 3]), 0.0), 255.0);
  const int co = (int)fmin(fmax(rint(attr[j * 3 + 1]), -255.0), 255.0);
  const int cg = (int)fmin(fmax(rint(attr[j * 3 + 2]), -255.0), 255.0);
  const int t = y - (cg >> 1), g = cg + t, b = t - (co >> 1), r = b + co;
  rgb[i * 3] = (uint8_t)min(max(r, 0), 255);
  rgb[i * 3 + 1] = (uint8_t)min(max(g, 0), 255);
  rgb[i * 3 + 2] = (uint8_t)min(max(b, 0), 255);
}

// ---------------------------------------------------------------------------------------------------------------- quantiser, symbols
// q[k][c] = rint(coef[order[k]][c] / step) (step 4), and the largest |q| of every subband
__global__ void __launch_bounds__(kThreads) quantize_kernel(const double* coef, const int32_t* order, const int32_t* subband, int64_t m,
                                                            double step, int32_t* q, int32_t* level_maxabs) {
  __shared__ int mx[kBins];
  if (threadIdx.x < kBins) mx[threadIdx.x] = 0;
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < m) {
    const int64_t j = order[k];
    int a = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = fmin(fmax(rint(coef[j * 3 + c] / step), -2147483647.0), 2147483647.0);
      const int qi = (int)v;
      q[k * 3 + c] = qi;
      a = max(a, abs(qi));
    }
    atomicMax(&mx[subband[j]], a);
  }
  __syncthreads();
  if (threadIdx.x < kBins && mx[threadIdx.x] > 0) atomicMax(&level_maxabs[threadIdx.x], mx[threadIdx.x]);
}

// symbol = q + amax of its subband, or the escape symbol 2 amax + 1 where |q| > amax
__global__ void __launch_bounds__(kThreads) symbols_kernel(const int32_t* q, const int32_t* order, const int32_t* subband, int64_t n,
                                                           const int32_t* amax, int16_t* sym) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const int a = amax[subband[order[k]]];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = q[k * 3 + c];
    sym[k * 3 + c] = (int16_t)(abs(v) <= a ? v + a : 2 * a + 1);
  }
}

// sums[subband][c] += min(|q|, amax[subband] + 1) over the rows k < n: the first moment the colour tables are fitted to, in integers.
// The rows come in subband order, so a wave almost always holds one subband: it then adds its 64 values up with lane shuffles
// and makes one LDS atomic per channel; a wave that straddles two subbands falls back to one atomic per lane.
__global__ void __launch_bounds__(kThreads) abs_sums_kernel(const int32_t* q, const int32_t* order, const int32_t* subband, int64_t n,
                                                            const int32_t* amax, unsigned long long* sums) {
  __shared__ unsigned int part[kBins * 3];                              // at most 256 x (AMAX_CAP + 1) per entry
  if (threadIdx.x < kBins * 3) part[threadIdx.x] = 0;
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = k < n;
  int l = -1;
  unsigned int a[3] = {0u, 0u, 0u};
  if (valid) {
    l = min(max(subband[order[k]], 0), kBins - 1);
    const unsigned int cap = (unsigned int)min(max(amax[l], 0), 2047) + 1u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = q[k * 3 + c];
      a[c] = min(v < 0 ? 0u - (unsigned int)v : (unsigned int)v, cap);
    }
  }
  const unsigned long long live = __ballot(valid);
  if (live) {                                                           // wave-uniform
    const int lref = __shfl(l, __ffsll((long long)live) - 1);
    if (__all(!valid || l == lref)) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        unsigned int v = a[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0 && v) atomicAdd(&part[lref * 3 + c], v);
      }
    } else if (valid) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (a[c]) atomicAdd(&part[l * 3 + c], a[c]);
    }
  }
  __syncthreads();
  if (threadIdx.x < kBins * 3 && part[threadIdx.x]) atomicAdd(&sums[threadIdx.x], (unsigned long long)part[threadIdx.x]);
}

__global__ void __launch_bounds__(kThreads) dequantize_kernel(const int16_t* sym, const int32_t* order, const int32_t* subband, int64_t n,
                                                              const int32_t* amax, double step, double* coef) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const int64_t j = order[k];
  const int a = amax[subband[j]];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s = sym[k * 3 + c];
    coef[j * 3 + c] = s > 2 * a ? 0.0 : (double)(s - a) * step;          // an escape: the patch list holds its value
  }
}

// patch[i] = (k * 3 + c, q): the escaped and the raw values
__global__ void __launch_bounds__(kThreads) patch_kernel(const int32_t* patch, int64_t n, const int32_t* order, int64_t m, double step,
                                                         double* coef) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t at = patch[i * 2];
  if (at < 0 || at >= m * 3) return;
  coef[(int64_t)order[at / 3] * 3 + at % 3] = (double)patch[i * 2 + 1] * step;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

bool shape_ok(int64_t m, int depth) { return m > 0 && m <= 0x7FFFFFFF && depth >= 0 && depth <= kMaxDepth; }

// the level from which the one-workgroup kernel takes over: the lowest l with no more than kTop leaves at levels >= l (DC included)
int top_level(const int64_t* level_counts, int nlev) {
  int64_t above = level_counts[nlev];
  int l0 = nlev;
  while (l0 > 0 && above + level_counts[l0 - 1] <= kTop) above += level_counts[--l0];
  return l0;
}

template <bool kInverse>
int run_transform(double* attr, int64_t m, int depth, const int32_t* left, const int32_t* w_right, const int32_t* subband,
                  const int32_t* order, const int64_t* level_counts, int fuse_top, int* launches, void* workspace, hipStream_t s) {
  const int nlev = 3 * depth;
  int64_t off[kBins + 1];
  off[0] = 0;
  int64_t total = 0;
  for (int l = 0; l <= nlev; ++l) { PCGC_REQUIRE(level_counts[l] >= 0, "pcgc_raht: negative level count"); off[l + 1] = off[l] + level_counts[l]; }
  total = off[nlev + 1];
  PCGC_REQUIRE(total == m && level_counts[nlev] == 1, "pcgc_raht: the level counts do not belong to a cloud of %lld points", (long long)m);
  const int l0 = fuse_top ? top_level(level_counts, nlev) : nlev;
  int count = 0;
  auto levels = [&](int l) {
    if (level_counts[l] == 0) return;
    hipLaunchKernelGGL(level_kernel<kInverse>, dim3(blocks_for(level_counts[l])), dim3(kThreads), 0, s, attr, order, off[l], level_counts[l],
                       left, w_right);
    ++count;
  };
  auto top = [&]() {
    if (l0 >= nlev) return;
    hipLaunchKernelGGL(top_kernel<kInverse>, dim3(1), dim3(kTop), 0, s, attr, order, off[l0], (int)(m - off[l0]), left, w_right, subband,
                       static_cast<int32_t*>(workspace), l0, nlev);
    ++count;
  };
  if (kInverse) {
    top();
    for (int l = l0 - 1; l >= 0; --l) levels(l);
  } else {
    for (int l = 0; l < l0; ++l) levels(l);
    top();
  }
  if (launches) *launches = count;
  return launch_ok(kInverse ? "raht inverse kernels" : "raht forward kernels");
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

// workspace: structure pass = the per-block subband histograms, then 512 bytes (level counts, refusal flag); the tree top = one
// int32 per leaf (pos).  The two uses never overlap in time.
size_t pcgc_raht_workspace_bytes(int64_t m) {
  if (m <= 0 || m > 0x7FFFFFFF) return 0;
  return std::max(align256((size_t)blocks_for(m) * kBins * sizeof(int32_t)) + 512, align256((size_t)m * sizeof(int32_t)));
}

int pcgc_raht_keys(const int32_t* points, int64_t m, int64_t* keys, pcgc_stream_t stream) {
  PCGC_REQUIRE(points && keys && m > 0, "pcgc_raht_keys: bad arguments");
  hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, (hipStream_t)stream, points, m, keys);
  return launch_ok("raht keys kernel");
}

int pcgc_raht_structure(const int64_t* sorted_keys, int64_t m, int depth, int32_t* subband, int32_t* left, int32_t* w_right,
                        int32_t* order, int64_t* level_counts, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(sorted_keys && subband && left && w_right && order && level_counts && workspace && shape_ok(m, depth),
               "pcgc_raht_structure: bad arguments");
  PCGC_REQUIRE(workspace_bytes >= pcgc_raht_workspace_bytes(m), "pcgc_raht_structure: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nlev = 3 * depth;
  const unsigned nblk = blocks_for(m);
  int32_t* block_hist = static_cast<int32_t*>(workspace);
  char* tail = static_cast<char*>(workspace) + align256((size_t)nblk * kBins * sizeof(int32_t));
  int64_t* counts_d = reinterpret_cast<int64_t*>(tail);
  int32_t* bad_d = reinterpret_cast<int32_t*>(tail + 448);
  static_assert(kBins * sizeof(int64_t) <= 448, "the level counts and the flag share 512 bytes");
  PCGC_CHECK_HIP(hipMemsetAsync(tail, 0, 512, s));
  hipLaunchKernelGGL(structure_kernel, dim3(nblk), dim3(kThreads), 0, s, sorted_keys, m, nlev, subband, left, w_right, block_hist, bad_d);
  hipLaunchKernelGGL(hist_scan_kernel, dim3(1), dim3(kScanSegs * 64), 0, s, block_hist, (int64_t)nblk, counts_d);
  int rc = launch_ok("raht structure kernels");
  if (rc) return rc;
  int64_t host[64] = {0};
  PCGC_CHECK_HIP(hipMemcpyAsync(host, tail, 512, hipMemcpyDeviceToHost, s));
  PCGC_CHECK_HIP(hipStreamSynchronize(s));
  int32_t bad;
  memcpy(&bad, reinterpret_cast<const char*>(host) + 448, sizeof(bad));
  PCGC_REQUIRE(!bad, "pcgc_raht_structure: the keys are not sorted, unique and below 2^%d", nlev);
  int64_t total = 0;
  for (int l = 0; l <= nlev; ++l) { level_counts[l] = host[l]; total += host[l]; }
  PCGC_REQUIRE(total == m && host[nlev] == 1, "pcgc_raht_structure: inconsistent level counts");
  hipLaunchKernelGGL(order_kernel, dim3(nblk), dim3(kThreads), 0, s, subband, m, nlev + 1, block_hist, order);
  return launch_ok("raht order kernel");
}

int pcgc_raht_forward(double* attr, int64_t m, int depth, const int32_t* left, const int32_t* w_right, const int32_t* subband,
                      const int32_t* order, const int64_t* level_counts, int fuse_top, int* launches, void* workspace,
                      size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(attr && left && w_right && subband && order && level_counts && workspace && shape_ok(m, depth),
               "pcgc_raht_forward: bad arguments");
  PCGC_REQUIRE(workspace_bytes >= pcgc_raht_workspace_bytes(m), "pcgc_raht_forward: workspace too small");
  return run_transform<false>(attr, m, depth, left, w_right, subband, order, level_counts, fuse_top, launches, workspace, (hipStream_t)stream);
}

int pcgc_raht_inverse(double* attr, int64_t m, int depth, const int32_t* left, const int32_t* w_right, const int32_t* subband,
                      const int32_t* order, const int64_t* level_counts, int fuse_top, int* launches, void* workspace,
                      size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(attr && left && w_right && subband && order && level_counts && workspace && shape_ok(m, depth),
               "pcgc_raht_inverse: bad arguments");
  PCGC_REQUIRE(workspace_bytes >= pcgc_raht_workspace_bytes(m), "pcgc_raht_inverse: workspace too small");
  return run_transform<true>(attr, m, depth, left, w_right, subband, order, level_counts, fuse_top, launches, workspace, (hipStream_t)stream);
}

int pcgc_raht_load_colors(const uint8_t* rgb, const int64_t* point_of_leaf, int64_t m, double* attr, pcgc_stream_t stream) {
  PCGC_REQUIRE(rgb && point_of_leaf && attr && m > 0, "pcgc_raht_load_colors: bad arguments");
  hipLaunchKernelGGL(load_colors_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, (hipStream_t)stream, rgb, point_of_leaf, m, attr);
  return launch_ok("raht load colours kernel");
}

int pcgc_raht_store_colors(const double* attr, const int64_t* point_of_leaf, int64_t m, uint8_t* rgb, pcgc_stream_t stream) {
  PCGC_REQUIRE(rgb && point_of_leaf && attr && m > 0, "pcgc_raht_store_colors: bad arguments");
  hipLaunchKernelGGL(store_colors_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, (hipStream_t)stream, attr, point_of_leaf, m, rgb);
  return launch_ok("raht store colours kernel");
}

int pcgc_raht_quantize(const double* coef, const int32_t* order, const int32_t* subband, int64_t m, double step, int32_t* q,
                       int32_t* level_maxabs, pcgc_stream_t stream) {
  PCGC_REQUIRE(coef && order && subband && q && level_maxabs && m > 0 && step > 0.0, "pcgc_raht_quantize: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemsetAsync(level_maxabs, 0, kBins * sizeof(int32_t), s));
  hipLaunchKernelGGL(quantize_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, s, coef, order, subband, m, step, q, level_maxabs);
  return launch_ok("raht quantise kernel");
}

int pcgc_raht_symbols(const int32_t* q, const int32_t* order, const int32_t* subband, int64_t n, const int32_t* amax, int16_t* symbols,
                      pcgc_stream_t stream) {
  PCGC_REQUIRE(n >= 0 && (n == 0 || (q && order && subband && amax && symbols)), "pcgc_raht_symbols: bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(symbols_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, q, order, subband, n, amax, symbols);
  return launch_ok("raht symbols kernel");
}

int pcgc_raht_abs_sums(const int32_t* q, const int32_t* order, const int32_t* subband, int64_t n, const int32_t* amax, int64_t* sums,
                       pcgc_stream_t stream) {
  PCGC_REQUIRE(sums && n >= 0 && (n == 0 || (q && order && subband && amax)), "pcgc_raht_abs_sums: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  static_assert(kBins * 3 <= kThreads, "one thread per (subband, channel) sum");
  PCGC_CHECK_HIP(hipMemsetAsync(sums, 0, kBins * 3 * sizeof(int64_t), s));
  if (n == 0) return 0;
  hipLaunchKernelGGL(abs_sums_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, q, order, subband, n, amax,
                     reinterpret_cast<unsigned long long*>(sums));
  return launch_ok("raht abs sums kernel");
}

int pcgc_raht_dequantize(const int16_t* symbols, int64_t n, const int32_t* patch, int64_t n_patch, const int32_t* order,
                         const int32_t* subband, const int32_t* amax, int64_t m, double step, double* coef, pcgc_stream_t stream) {
  PCGC_REQUIRE(order && subband && coef && m > 0 && n >= 0 && n <= m && n_patch >= 0 && step > 0.0 && (n == 0 || (symbols && amax)) &&
               (n_patch == 0 || patch), "pcgc_raht_dequantize: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (n < m) PCGC_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)m * 3 * sizeof(double), s));
  if (n) hipLaunchKernelGGL(dequantize_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, symbols, order, subband, n, amax, step, coef);
  if (n_patch) hipLaunchKernelGGL(patch_kernel, dim3(blocks_for(n_patch)), dim3(kThreads), 0, s, patch, n_patch, order, m, step, coef);
  return launch_ok("raht dequantise kernels");
}

}  // extern "C"
