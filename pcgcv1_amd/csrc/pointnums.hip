// Encoder-side choice of the per-cube point counts (.pointnums) that minimise the cube-local D1 of what the decoder,
// run unchanged at rho = 1, reconstructs (gfx950).
//
//   dataprocess/inout_points.py:147-179     select_voxels / get_adaptive_thres: the decoder keeps the voxels whose logit is
//                                           >= the k-th largest (ties included) -> S(k)
//   eval_ablation_studies.py:152-205        the rho search this replaces at the encoder (one rho for the whole cloud)
//
// Per cube, over the voxels with logit >= t_K (the K-th largest, K = the largest candidate count):
//   pn_compact_kernel   the occupied voxels P and the segment S(K), both in index order
//   pn_rank_kernel      the rank of every segment voxel under (logit descending, index ascending) by counting, and the
//                       end of its tie group (= m(k) for every k whose (k-1)-th ranked voxel lies in that group)
//   pn_bdist_kernel     per ranked voxel, the squared distance to the nearest occupied voxel (brute force over P)
//   pn_adist_kernel     per occupied voxel, its running minimum distance over the ranked list; every drop adds the change
//                       to a difference array (int64 atomics: exact, so the sum does not depend on their order)
//   pn_scan_kernel      prefix sums of both -> A and B at every rank
//   pn_gather_kernel    m(k), A(k) = A at rank m(k) - 1, B(k) likewise, k = 1 .. K
// and the selection's device part:
//   pn_sweep_kernel     per (cube, assignment): argmin over k of j A + (J - j) B (ties: smallest k), or a given k
//   pn_sum_kernel       per assignment: sum A, sum B, sum m over the cubes
// Everything is integer arithmetic: the curves and the sums are exact and deterministic.
//
// The point-to-plane (D2) curves (--pointnums d2) run the same two searches and measure each winner along a normal:
//   pn_owner_kernel / pn_nquant_kernel   the normal of every occupied voxel: that of its lowest-index input point (integer
//                       atomic min, then a gather), quantised to rint(1024 n / |n|), int16 x 4 in P's order
//   pn_bplane_kernel    pn_bdist_kernel's search carrying (distance, position in P); emits ((p* - v) . n_q(p*))^2
//   pn_aplane_kernel    pn_adist_kernel's running strict minimum; each change of the nearest voxel adds (new - old) plane error,
//                       of either sign, to the difference array
// compact, rank, scan, gather and the sweep serve both.
#include <climits>
#include "common.h"
#include "workspace.h"

namespace pcgc {
namespace {

constexpr int kTile = 256;

// ascending floats -> ascending unsigned, with -0.0 and +0.0 folded into one key (they compare equal in the decoder's >=)
__device__ __forceinline__ uint32_t pn_key(float f) {
  if (f == 0.0f) f = 0.0f;
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// voxel index (NDHWC, one channel: ((d * cs) + h) * cs + w) -> packed (d, h, w), 8 bits each (cs <= 256)
__device__ __forceinline__ uint32_t pn_pack(int32_t i, int cs) {
  const uint32_t w = (uint32_t)(i % cs), t = (uint32_t)(i / cs);
  return (w << 16) | ((t % (uint32_t)cs) << 8) | (t / (uint32_t)cs);
}
__device__ __forceinline__ int pn_d2(uint32_t a, uint32_t b) {
  const int dx = (int)(a & 255u) - (int)(b & 255u);
  const int dy = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u);
  const int dz = (int)(a >> 16) - (int)(b >> 16);
  return dx * dx + dy * dy + dz * dz;
}

// counts of one cube: occupied voxels and voxels at or above the threshold
__global__ void __launch_bounds__(1024) pn_count_kernel(const float* x, const float* logits, const float* thr, int64_t vox,
                                                        int32_t* n_pts, int32_t* n_seg) {
  __shared__ uint32_t sh[2];
  const int b = blockIdx.x;
  const float* xc = x + (int64_t)b * vox;
  const float* lc = logits + (int64_t)b * vox;
  const float t = thr[b];
  if (threadIdx.x == 0) { sh[0] = 0; sh[1] = 0; }
  __syncthreads();
  uint32_t cp = 0, cs = 0;
  for (int64_t i = threadIdx.x; i < vox; i += 1024) {
    cp += xc[i] > 0.0f ? 1u : 0u;
    cs += lc[i] >= t ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cp += __shfl_xor(cp, o); cs += __shfl_xor(cs, o); }
  if ((threadIdx.x & 63) == 0) { atomicAdd(&sh[0], cp); atomicAdd(&sh[1], cs); }
  __syncthreads();
  if (threadIdx.x == 0) { n_pts[b] = (int32_t)sh[0]; n_seg[b] = (int32_t)sh[1]; }
}

// stream compaction in index order: a wave ballots, its lanes take positions by popcount below them, waves in wave order
__global__ void __launch_bounds__(1024) pn_compact_kernel(const float* x, const float* logits, const float* thr, int64_t vox,
                                                          const int64_t* pts_off, const int64_t* seg_off, int32_t* pts,
                                                          uint32_t* seg_key, int32_t* seg_idx) {
  __shared__ uint32_t wp[16], ws[16];
  __shared__ uint32_t base[2];
  const int b = blockIdx.x;
  const float* xc = x + (int64_t)b * vox;
  const float* lc = logits + (int64_t)b * vox;
  const float t = thr[b];
  const int64_t p0 = pts_off[b], np_ = pts_off[b + 1] - p0;
  const int64_t s0 = seg_off[b], ns = seg_off[b + 1] - s0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) { base[0] = 0; base[1] = 0; }
  __syncthreads();
  for (int64_t t0 = 0; t0 < vox; t0 += 1024) {
    const int64_t i = t0 + threadIdx.x;
    const bool in = i < vox;
    const float l = in ? lc[i] : 0.0f;
    const bool p = in && xc[i] > 0.0f, s = in && l >= t;
    const uint64_t bp = __ballot(p), bs = __ballot(s);
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (lane == 0) { wp[w] = (uint32_t)__popcll(bp); ws[w] = (uint32_t)__popcll(bs); }
    __syncthreads();
    uint32_t op = base[0], os = base[1];
    for (int k = 0; k < w; ++k) { op += wp[k]; os += ws[k]; }
    op += (uint32_t)__popcll(bp & below);
    os += (uint32_t)__popcll(bs & below);
    if (p && (int64_t)op < np_) pts[p0 + op] = (int32_t)i;
    if (s && (int64_t)os < ns) { seg_key[s0 + os] = pn_key(l); seg_idx[s0 + os] = (int32_t)i; }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t a = 0, c = 0;
      for (int k = 0; k < 16; ++k) { a += wp[k]; c += ws[k]; }
      base[0] += a; base[1] += c;
    }
    __syncthreads();
  }
}

// blocks[2 g] = cube, blocks[2 g + 1] = first element of block g (element lists of every cube cut into kTile pieces)
__global__ void __launch_bounds__(kTile) pn_rank_kernel(const int32_t* blocks, const int64_t* seg_off, const uint32_t* seg_key,
                                                        const int32_t* seg_idx, int32_t* sorted_idx, int32_t* gend) {
  __shared__ uint32_t tk[kTile];
  __shared__ int32_t ti[kTile];
  const int b = blocks[2 * blockIdx.x], start = blocks[2 * blockIdx.x + 1];
  const int64_t s0 = seg_off[b];
  const int M = (int)(seg_off[b + 1] - s0);
  const int v = start + threadIdx.x;
  const bool mine = v < M;
  const uint32_t kv = mine ? seg_key[s0 + v] : 0u;
  const int32_t iv = mine ? seg_idx[s0 + v] : 0;
  int gt = 0, eq = 0, eqlo = 0;
  for (int t0 = 0; t0 < M; t0 += kTile) {
    const int u = t0 + threadIdx.x;
    if (u < M) { tk[threadIdx.x] = seg_key[s0 + u]; ti[threadIdx.x] = seg_idx[s0 + u]; }
    __syncthreads();
    const int n = min(kTile, M - t0);
    for (int q = 0; q < n; ++q) {
      const uint32_t ku = tk[q];
      gt += ku > kv ? 1 : 0;
      const bool e = ku == kv;
      eq += e ? 1 : 0;
      eqlo += (e && ti[q] < iv) ? 1 : 0;
    }
    __syncthreads();
  }
  const int r = gt + eqlo;                       // a permutation of 0 .. M-1: (key, index) pairs are distinct
  if (mine && r < M) {
    sorted_idx[s0 + r] = iv;
    gend[s0 + r] = gt + eq;
  }
}

// per ranked voxel: squared distance to the nearest occupied voxel of the cube
__global__ void __launch_bounds__(kTile) pn_bdist_kernel(const int32_t* blocks, const int64_t* seg_off, const int64_t* pts_off,
                                                         const int32_t* sorted_idx, const int32_t* pts, int cs, int64_t* dB) {
  __shared__ uint32_t tp[kTile];
  const int b = blocks[2 * blockIdx.x], start = blocks[2 * blockIdx.x + 1];
  const int64_t s0 = seg_off[b], p0 = pts_off[b];
  const int M = (int)(seg_off[b + 1] - s0), N = (int)(pts_off[b + 1] - p0);
  const int r = start + threadIdx.x;
  const bool mine = r < M;
  const uint32_t cv = pn_pack(mine ? sorted_idx[s0 + r] : 0, cs);
  int best = INT_MAX;
  for (int t0 = 0; t0 < N; t0 += kTile) {
    const int u = t0 + threadIdx.x;
    if (u < N) tp[threadIdx.x] = pn_pack(pts[p0 + u], cs);
    __syncthreads();
    const int n = min(kTile, N - t0);
    for (int q = 0; q < n; ++q) best = min(best, pn_d2(cv, tp[q]));
    __syncthreads();
  }
  if (mine) dB[s0 + r] = N > 0 ? (int64_t)best : 0;
}

// per occupied voxel: running minimum of its distance over the ranked list; each drop (and the first value) is added to
// the difference array at that rank
__global__ void __launch_bounds__(kTile) pn_adist_kernel(const int32_t* blocks, const int64_t* seg_off, const int64_t* pts_off,
                                                         const int32_t* sorted_idx, const int32_t* pts, int cs, int64_t* dA) {
  __shared__ uint32_t tv[kTile];
  const int b = blocks[2 * blockIdx.x], start = blocks[2 * blockIdx.x + 1];
  const int64_t s0 = seg_off[b], p0 = pts_off[b];
  const int M = (int)(seg_off[b + 1] - s0), N = (int)(pts_off[b + 1] - p0);
  const int p = start + threadIdx.x;
  const bool mine = p < N;
  const uint32_t cp = pn_pack(mine ? pts[p0 + p] : 0, cs);
  int cur = INT_MAX;
  unsigned long long* da = reinterpret_cast<unsigned long long*>(dA + s0);
  for (int t0 = 0; t0 < M; t0 += kTile) {
    const int u = t0 + threadIdx.x;
    if (u < M) tv[threadIdx.x] = pn_pack(sorted_idx[s0 + u], cs);
    __syncthreads();
    if (mine) {
      const int n = min(kTile, M - t0);
      for (int q = 0; q < n; ++q) {
        const int d = pn_d2(cp, tv[q]);
        if (d < cur) {
          const int64_t delta = cur == INT_MAX ? (int64_t)d : (int64_t)d - (int64_t)cur;
          atomicAdd(da + t0 + q, (unsigned long long)delta);       // two's complement: a negative step wraps exactly
          cur = d;
        }
      }
    }
    __syncthreads();
  }
}

// inclusive prefix sums of dA and dB over one cube's segment, in place (one workgroup per cube, 1024-element tiles)
__global__ void __launch_bounds__(1024) pn_scan_kernel(const int64_t* seg_off, int64_t* dA, int64_t* dB) {
  __shared__ int64_t wa[16], wb[16];
  __shared__ int64_t carry[2];
  const int b = blockIdx.x;
  const int64_t s0 = seg_off[b], M = seg_off[b + 1] - s0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) { carry[0] = 0; carry[1] = 0; }
  __syncthreads();
  for (int64_t t0 = 0; t0 < M; t0 += 1024) {
    const int64_t i = t0 + threadIdx.x;
    int64_t a = i < M ? dA[s0 + i] : 0, c = i < M ? dB[s0 + i] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t ya = __shfl_up(a, o), yc = __shfl_up(c, o);
      if (lane >= o) { a += ya; c += yc; }
    }
    if (lane == 63) { wa[w] = a; wb[w] = c; }
    __syncthreads();
    int64_t ca = carry[0], cc = carry[1];
    for (int k = 0; k < w; ++k) { ca += wa[k]; cc += wb[k]; }
    if (i < M) { dA[s0 + i] = a + ca; dB[s0 + i] = c + cc; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t sa = 0, sc = 0;
      for (int k = 0; k < 16; ++k) { sa += wa[k]; sc += wb[k]; }
      carry[0] += sa; carry[1] += sc;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kTile) pn_gather_kernel(const int64_t* seg_off, const int64_t* curve_off, const int32_t* gend,
                                                          const int64_t* pA, const int64_t* pB, int32_t* m, int64_t* A,
                                                          int64_t* Bc) {
  const int b = blockIdx.x;
  const int64_t s0 = seg_off[b], M = seg_off[b + 1] - s0;
  const int64_t c0 = curve_off[b], K = curve_off[b + 1] - c0;
  for (int64_t k = threadIdx.x; k < K && k < M; k += kTile) {
    int64_t g = gend[s0 + k];
    g = g < 1 ? 1 : (g > M ? M : g);
    m[c0 + k] = (int32_t)g;
    A[c0 + k] = pA[s0 + g - 1];
    Bc[c0 + k] = pB[s0 + g - 1];
  }
}

// one (cube, assignment) per workgroup: a < n_sweep -> j = a, argmin over k of j A + (J - j) B; else the given k
__global__ void __launch_bounds__(kTile) pn_sweep_kernel(const int32_t* m, const int64_t* A, const int64_t* Bc,
                                                         const int64_t* curve_off, int B, int J, const int32_t* fixed_k,
                                                         int32_t* k_out, int64_t* picks) {
  __shared__ int64_t sv[kTile / 64];
  __shared__ int32_t sk[kTile / 64];
  __shared__ int32_t pick_k;
  const int b = blockIdx.x, a = blockIdx.y;
  const int64_t c0 = curve_off[b], K = curve_off[b + 1] - c0;
  if (a <= J) {
    const int64_t wa = a, wb = J - a;
    int64_t bv = LLONG_MAX;
    int32_t bk = INT_MAX;
    for (int64_t k = threadIdx.x; k < K; k += kTile) {
      const int64_t v = wa * A[c0 + k] + wb * Bc[c0 + k];
      if (v < bv) { bv = v; bk = (int32_t)k; }                 // strided ascending k: the first minimum is the smallest k
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t ov = __shfl_xor(bv, o);
      const int32_t ok = __shfl_xor(bk, o);
      if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; sk[threadIdx.x >> 6] = bk; }
    __syncthreads();
    if (threadIdx.x == 0) {
      bv = sv[0]; bk = sk[0];
      for (int q = 1; q < kTile / 64; ++q)
        if (sv[q] < bv || (sv[q] == bv && sk[q] < bk)) { bv = sv[q]; bk = sk[q]; }
      pick_k = bk == INT_MAX ? 0 : bk + 1;
    }
  } else if (threadIdx.x == 0) {
    int32_t k = fixed_k[(int64_t)(a - J - 1) * B + b];
    pick_k = k < 1 ? 1 : (k > K ? (int32_t)K : k);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t k = pick_k;
    const int64_t o = (int64_t)a * B + b;
    k_out[o] = k;
    const bool ok = k >= 1 && k <= K;
    picks[3 * o + 0] = ok ? A[c0 + k - 1] : 0;
    picks[3 * o + 1] = ok ? Bc[c0 + k - 1] : 0;
    picks[3 * o + 2] = ok ? (int64_t)m[c0 + k - 1] : 0;
  }
}

__global__ void __launch_bounds__(kTile) pn_sum_kernel(const int64_t* picks, int B, int64_t* sums) {
  __shared__ int64_t sh[3][kTile / 64];
  const int a = blockIdx.x;
  int64_t s[3] = {0, 0, 0};
  for (int b = threadIdx.x; b < B; b += kTile)
    for (int q = 0; q < 3; ++q) s[q] += picks[3 * ((int64_t)a * B + b) + q];
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
  }
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < 3; ++q) sh[q][threadIdx.x >> 6] = s[q];
  __syncthreads();
  if (threadIdx.x < 3) {
    int64_t t = 0;
    for (int w = 0; w < kTile / 64; ++w) t += sh[threadIdx.x][w];
    sums[3 * a + threadIdx.x] = t;
  }
}

// ---- point-to-plane (D2) curves: the same two searches, each winner measured along the occupied voxel's normal ----
// A voxel's normal is int16 x 4 (nx, ny, nz, 0), |component| <= 1024, read as one int2: x = nx | ny << 16, y = nz.
__device__ __forceinline__ int64_t pn_plane(uint32_t a, uint32_t b, int2 n) {
  const int dx = (int)(a & 255u) - (int)(b & 255u);
  const int dy = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u);
  const int dz = (int)(a >> 16) - (int)(b >> 16);
  const int dot = dx * (int)(int16_t)(n.x & 0xffff) + dy * (n.x >> 16) + dz * (int)(int16_t)(n.y & 0xffff);   // <= 3 255 1024
  return (int64_t)dot * (int64_t)dot;
}

// per ranked voxel: the nearest occupied voxel (ties: the smallest voxel index = the first in P's order, kept by the strict
// <), then the squared distance to that voxel's plane
__global__ void __launch_bounds__(kTile) pn_bplane_kernel(const int32_t* blocks, const int64_t* seg_off, const int64_t* pts_off,
                                                          const int32_t* sorted_idx, const int32_t* pts, const int2* vn, int cs,
                                                          int64_t* dB) {
  __shared__ uint32_t tp[kTile];
  const int b = blocks[2 * blockIdx.x], start = blocks[2 * blockIdx.x + 1];
  const int64_t s0 = seg_off[b], p0 = pts_off[b];
  const int M = (int)(seg_off[b + 1] - s0), N = (int)(pts_off[b + 1] - p0);
  const int r = start + threadIdx.x;
  const bool mine = r < M;
  const uint32_t cv = pn_pack(mine ? sorted_idx[s0 + r] : 0, cs);
  int best = INT_MAX, bi = 0;
  for (int t0 = 0; t0 < N; t0 += kTile) {
    const int u = t0 + threadIdx.x;
    if (u < N) tp[threadIdx.x] = pn_pack(pts[p0 + u], cs);
    __syncthreads();
    const int n = min(kTile, N - t0);
    for (int q = 0; q < n; ++q) {
      const int d = pn_d2(cv, tp[q]);
      if (d < best) { best = d; bi = t0 + q; }
    }
    __syncthreads();
  }
  if (mine) dB[s0 + r] = N > 0 ? pn_plane(pn_pack(pts[p0 + bi], cs), cv, vn[p0 + bi]) : 0;
}

// per occupied voxel: its nearest voxel over the ranked list changes only on a strict drop of the distance (ties: the lowest
// rank); every change adds (new - old) plane error, of either sign, to the difference array at that rank
__global__ void __launch_bounds__(kTile) pn_aplane_kernel(const int32_t* blocks, const int64_t* seg_off, const int64_t* pts_off,
                                                          const int32_t* sorted_idx, const int32_t* pts, const int2* vn, int cs,
                                                          int64_t* dA) {
  __shared__ uint32_t tv[kTile];
  const int b = blocks[2 * blockIdx.x], start = blocks[2 * blockIdx.x + 1];
  const int64_t s0 = seg_off[b], p0 = pts_off[b];
  const int M = (int)(seg_off[b + 1] - s0), N = (int)(pts_off[b + 1] - p0);
  const int p = start + threadIdx.x;
  const bool mine = p < N;
  const uint32_t cp = pn_pack(mine ? pts[p0 + p] : 0, cs);
  const int2 nq = mine ? vn[p0 + p] : make_int2(0, 0);
  int cur = INT_MAX;
  int64_t cur_e = 0;
  unsigned long long* da = reinterpret_cast<unsigned long long*>(dA + s0);
  for (int t0 = 0; t0 < M; t0 += kTile) {
    const int u = t0 + threadIdx.x;
    if (u < M) tv[threadIdx.x] = pn_pack(sorted_idx[s0 + u], cs);
    __syncthreads();
    if (mine) {
      const int n = min(kTile, M - t0);
      for (int q = 0; q < n; ++q) {
        const int d = pn_d2(cp, tv[q]);
        if (d < cur) {
          const int64_t e = pn_plane(tv[q], cp, nq);
          if (e != cur_e) atomicAdd(da + t0 + q, (unsigned long long)(e - cur_e));   // two's complement: exact in any order
          cur = d;
          cur_e = e;
        }
      }
    }
    __syncthreads();
  }
}

// voxel normals: point i (key = cube * cs^3 + voxel, < 0: a point of a dropped cube) finds its voxel in the sorted distinct keys
// and leaves the smallest i there
__global__ void __launch_bounds__(kTile) pn_owner_kernel(const int64_t* point_key, int64_t n_points, const int64_t* vox_key,
                                                         int64_t n_vox, int32_t* owner) {
  const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (i >= n_points) return;
  const int64_t key = point_key[i];
  if (key < 0) return;
  int64_t lo = 0, hi = n_vox;                                    // first slot with vox_key >= key
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (vox_key[mid] < key) lo = mid + 1; else hi = mid;
  }
  if (lo < n_vox && vox_key[lo] == key) atomicMin(&owner[lo], (int32_t)i);
}

// n_q = rint(1024 n / |n|) in float64, half to even; a zero or non-finite normal (or a voxel no point claimed) -> (0, 0, 0)
__global__ void __launch_bounds__(kTile) pn_nquant_kernel(const int32_t* owner, const float* normals, int64_t n_points,
                                                          int64_t n_vox, int16_t* out) {
  const int64_t s = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (s >= n_vox) return;
  const int64_t i = owner[s];
  int q[3] = {0, 0, 0};
  if (i >= 0 && i < n_points) {
    const double x = (double)normals[3 * i], y = (double)normals[3 * i + 1], z = (double)normals[3 * i + 2];
    const double len = sqrt(x * x + y * y + z * z);
    if (isfinite(x) && isfinite(y) && isfinite(z) && len > 0.0) {
      q[0] = (int)rint(1024.0 * x / len);
      q[1] = (int)rint(1024.0 * y / len);
      q[2] = (int)rint(1024.0 * z / len);
    }
  }
  out[4 * s] = (int16_t)q[0]; out[4 * s + 1] = (int16_t)q[1]; out[4 * s + 2] = (int16_t)q[2]; out[4 * s + 3] = 0;
}

struct CurvesWs {
  int64_t *dA, *dB;          // [total_seg]
  uint32_t* seg_key;         // [total_seg], as are the next three
  int32_t *seg_idx, *sorted_idx, *gend;
  int32_t* pts;              // [max(total_pts, 1)]
  size_t bytes;
};

CurvesWs curves_layout(int64_t total_seg, int64_t total_pts, void* workspace) {
  Carver c(workspace);
  CurvesWs w;
  w.dA = c.take<int64_t>((size_t)total_seg);
  w.dB = c.take<int64_t>((size_t)total_seg);
  w.seg_key = c.take<uint32_t>((size_t)total_seg);
  w.seg_idx = c.take<int32_t>((size_t)total_seg);
  w.sorted_idx = c.take<int32_t>((size_t)total_seg);
  w.gend = c.take<int32_t>((size_t)total_seg);
  w.pts = c.take<int32_t>((size_t)(total_pts > 0 ? total_pts : 1));
  w.bytes = c.bytes();
  return w;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_pointnums_count(const float* x, const float* logits, const int32_t* k_max, int B, int cube_size, float* thresholds,
                         int32_t* n_pts, int32_t* n_seg, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && logits && k_max && thresholds && n_pts && n_seg && B > 0 && cube_size >= 1 && cube_size <= 256,
               "pcgc_pointnums_count: bad arguments");
  const int64_t vox = (int64_t)cube_size * cube_size * cube_size;
  int rc = pcgc_topk_threshold(logits, k_max, B, vox, 0, 0.0f, thresholds, nullptr, nullptr, 0, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(pn_count_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, logits, thresholds, vox, n_pts, n_seg);
  return launch_ok("pn_count_kernel");
}

size_t pcgc_pointnums_curves_workspace_bytes(int64_t total_seg, int64_t total_pts) {
  return curves_layout(total_seg, total_pts, nullptr).bytes;
}

int pcgc_pointnums_curves(const float* x, const float* logits, const float* thresholds, int B, int cube_size,
                          const int64_t* pts_off, const int64_t* seg_off, const int64_t* curve_off, int64_t total_seg,
                          int64_t total_pts, const int32_t* seg_blocks, int n_seg_blocks, const int32_t* pts_blocks,
                          int n_pts_blocks, int32_t* m, int64_t* A, int64_t* Bc, void* workspace, size_t workspace_bytes,
                          pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && logits && thresholds && pts_off && seg_off && curve_off && m && A && Bc && B > 0 && cube_size >= 1 &&
                   cube_size <= 256 && total_seg >= 0 && total_seg < ((int64_t)1 << 31) && total_pts >= 0 &&
                   n_seg_blocks >= 0 && n_pts_blocks >= 0 && (n_seg_blocks == 0 || seg_blocks) &&
                   (n_pts_blocks == 0 || pts_blocks),
               "pcgc_pointnums_curves: bad arguments");
  const CurvesWs w = curves_layout(total_seg, total_pts, workspace);
  PCGC_REQUIRE(workspace && workspace_bytes >= w.bytes, "pcgc_pointnums_curves: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t vox = (int64_t)cube_size * cube_size * cube_size;
  PCGC_CHECK_HIP(hipMemsetAsync(w.dA, 0, 8 * (size_t)total_seg, s));
  hipLaunchKernelGGL(pn_compact_kernel, dim3(B), dim3(1024), 0, s, x, logits, thresholds, vox, pts_off, seg_off, w.pts,
                     w.seg_key, w.seg_idx);
  if (int rc = launch_ok("pn_compact_kernel")) return rc;
  if (n_seg_blocks) {
    hipLaunchKernelGGL(pn_rank_kernel, dim3(n_seg_blocks), dim3(kTile), 0, s, seg_blocks, seg_off, w.seg_key, w.seg_idx,
                       w.sorted_idx, w.gend);
    if (int rc = launch_ok("pn_rank_kernel")) return rc;
    hipLaunchKernelGGL(pn_bdist_kernel, dim3(n_seg_blocks), dim3(kTile), 0, s, seg_blocks, seg_off, pts_off, w.sorted_idx,
                       w.pts, cube_size, w.dB);
    if (int rc = launch_ok("pn_bdist_kernel")) return rc;
  }
  if (n_pts_blocks) {
    hipLaunchKernelGGL(pn_adist_kernel, dim3(n_pts_blocks), dim3(kTile), 0, s, pts_blocks, seg_off, pts_off, w.sorted_idx,
                       w.pts, cube_size, w.dA);
    if (int rc = launch_ok("pn_adist_kernel")) return rc;
  }
  hipLaunchKernelGGL(pn_scan_kernel, dim3(B), dim3(1024), 0, s, seg_off, w.dA, w.dB);
  if (int rc = launch_ok("pn_scan_kernel")) return rc;
  hipLaunchKernelGGL(pn_gather_kernel, dim3(B), dim3(kTile), 0, s, seg_off, curve_off, w.gend, w.dA, w.dB, m, A, Bc);
  return launch_ok("pn_gather_kernel");
}

size_t pcgc_pointnums_normals_workspace_bytes(int64_t n_vox) { return align256(4 * (size_t)(n_vox > 0 ? n_vox : 1)); }

int pcgc_pointnums_normals(const int64_t* point_key, const float* normals, int64_t n_points, const int64_t* vox_key,
                           int64_t n_vox, int16_t* vox_normals, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  if (n_vox == 0) return 0;
  PCGC_REQUIRE(point_key && normals && vox_key && vox_normals && n_points > 0 && n_points < 0x7f7f7f7f && n_vox > 0 &&
                   n_vox <= n_points,
               "pcgc_pointnums_normals: bad arguments");
  PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_pointnums_normals_workspace_bytes(n_vox),
               "pcgc_pointnums_normals: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int32_t* owner = (int32_t*)workspace;
  PCGC_CHECK_HIP(hipMemsetAsync(owner, 0x7f, 4 * (size_t)n_vox, s));           // 0x7f7f7f7f: above every point index
  hipLaunchKernelGGL(pn_owner_kernel, dim3((unsigned)((n_points + kTile - 1) / kTile)), dim3(kTile), 0, s, point_key, n_points,
                     vox_key, n_vox, owner);
  if (int rc = launch_ok("pn_owner_kernel")) return rc;
  hipLaunchKernelGGL(pn_nquant_kernel, dim3((unsigned)((n_vox + kTile - 1) / kTile)), dim3(kTile), 0, s, (const int32_t*)owner,
                     normals, n_points, n_vox, vox_normals);
  return launch_ok("pn_nquant_kernel");
}

size_t pcgc_pointnums_curves_d2_workspace_bytes(int64_t total_seg, int64_t total_pts) {
  return curves_layout(total_seg, total_pts, nullptr).bytes;
}

int pcgc_pointnums_curves_d2(const float* x, const float* logits, const float* thresholds, const int16_t* vox_normals, int B,
                             int cube_size, const int64_t* pts_off, const int64_t* seg_off, const int64_t* curve_off,
                             int64_t total_seg, int64_t total_pts, const int32_t* seg_blocks, int n_seg_blocks,
                             const int32_t* pts_blocks, int n_pts_blocks, int32_t* m, int64_t* A2, int64_t* B2, void* workspace,
                             size_t workspace_bytes, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && logits && thresholds && pts_off && seg_off && curve_off && m && A2 && B2 && B > 0 && cube_size >= 1 &&
                   cube_size <= 256 && total_seg >= 0 && total_seg < ((int64_t)1 << 31) && total_pts >= 0 &&
                   n_seg_blocks >= 0 && n_pts_blocks >= 0 && (n_seg_blocks == 0 || seg_blocks) &&
                   (n_pts_blocks == 0 || pts_blocks) && (total_pts == 0 || vox_normals) && ((uintptr_t)vox_normals & 7) == 0,
               "pcgc_pointnums_curves_d2: bad arguments");
  const CurvesWs w = curves_layout(total_seg, total_pts, workspace);
  PCGC_REQUIRE(workspace && workspace_bytes >= w.bytes, "pcgc_pointnums_curves_d2: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t vox = (int64_t)cube_size * cube_size * cube_size;
  const int2* vn = reinterpret_cast<const int2*>(vox_normals);
  PCGC_CHECK_HIP(hipMemsetAsync(w.dA, 0, 8 * (size_t)total_seg, s));
  hipLaunchKernelGGL(pn_compact_kernel, dim3(B), dim3(1024), 0, s, x, logits, thresholds, vox, pts_off, seg_off, w.pts,
                     w.seg_key, w.seg_idx);
  if (int rc = launch_ok("pn_compact_kernel")) return rc;
  if (n_seg_blocks) {
    hipLaunchKernelGGL(pn_rank_kernel, dim3(n_seg_blocks), dim3(kTile), 0, s, seg_blocks, seg_off, w.seg_key, w.seg_idx,
                       w.sorted_idx, w.gend);
    if (int rc = launch_ok("pn_rank_kernel")) return rc;
    hipLaunchKernelGGL(pn_bplane_kernel, dim3(n_seg_blocks), dim3(kTile), 0, s, seg_blocks, seg_off, pts_off, w.sorted_idx,
                       w.pts, vn, cube_size, w.dB);
    if (int rc = launch_ok("pn_bplane_kernel")) return rc;
  }
  if (n_pts_blocks) {
    hipLaunchKernelGGL(pn_aplane_kernel, dim3(n_pts_blocks), dim3(kTile), 0, s, pts_blocks, seg_off, pts_off, w.sorted_idx,
                       w.pts, vn, cube_size, w.dA);
    if (int rc = launch_ok("pn_aplane_kernel")) return rc;
  }
  hipLaunchKernelGGL(pn_scan_kernel, dim3(B), dim3(1024), 0, s, seg_off, w.dA, w.dB);
  if (int rc = launch_ok("pn_scan_kernel")) return rc;
  hipLaunchKernelGGL(pn_gather_kernel, dim3(B), dim3(kTile), 0, s, seg_off, curve_off, w.gend, w.dA, w.dB, m, A2, B2);
  return launch_ok("pn_gather_kernel");
}

size_t pcgc_pointnums_sweep_workspace_bytes(int B, int n_assign) { return 24 * (size_t)B * (size_t)n_assign; }

int pcgc_pointnums_sweep(const int32_t* m, const int64_t* A, const int64_t* Bc, const int64_t* curve_off, int B, int J,
                         const int32_t* fixed_k, int L, int32_t* k_out, int64_t* sums, void* workspace,
                         size_t workspace_bytes, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(m && A && Bc && curve_off && k_out && sums && B > 0 && J >= 0 && J <= 1024 && L >= 0 && (L == 0 || fixed_k),
               "pcgc_pointnums_sweep: bad arguments");
  const int n_assign = J + 1 + L;
  PCGC_REQUIRE(n_assign <= 65535, "pcgc_pointnums_sweep: too many assignments");
  PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_pointnums_sweep_workspace_bytes(B, n_assign),
               "pcgc_pointnums_sweep: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int64_t* picks = (int64_t*)workspace;
  hipLaunchKernelGGL(pn_sweep_kernel, dim3(B, n_assign), dim3(kTile), 0, s, m, A, Bc, curve_off, B, J, fixed_k, k_out, picks);
  if (int rc = launch_ok("pn_sweep_kernel")) return rc;
  hipLaunchKernelGGL(pn_sum_kernel, dim3(n_assign), dim3(kTile), 0, s, (const int64_t*)picks, B, sums);
  return launch_ok("pn_sum_kernel");
}

}  // extern "C"
