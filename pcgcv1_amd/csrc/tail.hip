// Decoder-tail and loss kernels (gfx950): adaptive top-k threshold, BCE sums,
// device voxelisation, D1 / D2 distortion (on the voxel grid of voxel_grid.h).
//
//   dataprocess/inout_points.py:147-179  select_voxels / get_adaptive_thres
//   loss.py:8-33                         get_bce_loss
//   loss.py:35-78                        get_confusion_matrix / get_classify_metrics
//   loss.py:83-93                        get_focal_loss
//   dataprocess/inout_points.py:116-132  points2voxels
#include <algorithm>
#include "loss_sums.h"
#include "common.h"
#include "voxel_grid.h"

namespace pcgc {

__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // ascending floats -> ascending unsigned
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// One workgroup per cube: exact k-th largest by 4-pass MSB radix select over the
// candidates (values > -2.0, or all voxels when fewer than k of those), then the
// >= threshold mask.  Integer LDS atomics only => deterministic, bit-exact.
__global__ void __launch_bounds__(1024) topk_kernel(const float* x, const int32_t* k_per_cube, int64_t vox, int use_fixed,
                                                    float fixed_thres, float* thresholds, uint8_t* mask) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh_cnt;
  __shared__ uint32_t sh_prefix, sh_rank;
  const int b = blockIdx.x;
  const float* xc = x + (int64_t)b * vox;
  float thr = fixed_thres;
  if (!use_fixed) {
    if (threadIdx.x == 0) sh_cnt = 0;
    __syncthreads();
    uint32_t c = 0;
    for (int64_t i = threadIdx.x; i < vox; i += 1024) c += (xc[i] > -2.0f) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sh_cnt, c);
    __syncthreads();
    const uint32_t cnt = sh_cnt;
    const int64_t k = k_per_cube[b];
    const bool all = (int64_t)cnt < k;
    const int64_t total = all ? vox : (int64_t)cnt;
    // sorted ascending: values[-k]  ->  rank total-k; k == 0 -> values[0]; k > total is an IndexError in the
    // reference, clamped to rank 0 here
    int64_t r64 = (k <= 0 || k > total) ? 0 : total - k;
    if (threadIdx.x == 0) { sh_prefix = 0; sh_rank = (uint32_t)r64; }
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 256; i += 1024) hist[i] = 0;
      __syncthreads();
      const uint32_t prefix = sh_prefix;
      const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
      for (int64_t i = threadIdx.x; i < vox; i += 1024) {
        const float f = xc[i];
        if (all || f > -2.0f) {
          const uint32_t key = order_key(f);
          if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t r = sh_rank, cum = 0;
        int bin = 0;
        for (; bin < 256; ++bin) {
          if (cum + hist[bin] > r) break;
          cum += hist[bin];
        }
        if (bin > 255) bin = 255;
        sh_rank = r - cum;
        sh_prefix = prefix | ((uint32_t)bin << shift);
      }
      __syncthreads();
    }
    thr = key_to_float(sh_prefix);
  }
  if (threadIdx.x == 0) thresholds[b] = thr;
  if (mask) {
    uint8_t* mc = mask + (int64_t)b * vox;
    for (int64_t i = threadIdx.x; i < vox; i += 1024) mc[i] = (xc[i] >= thr) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
// BCE sums, deterministic two-stage reduction in double
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bce_partial_kernel(const float* pred, const float* label, int64_t n, double* partial) {
  __shared__ double sh[4][4];
  bce_partial_body(pred, label, n, partial, blockIdx.x, gridDim.x, sh);
}
__global__ void bce_final_kernel(const double* partial, int nblocks, double* sums4) {
  __shared__ double sh[64];
  bce_final_body(partial, nblocks, sums4, sh);
}

// ---------------------------------------------------------------------------
// Classification counts (loss.py:35-78): TP / FP / FN of (pred > th) against (label > th).  A wavefront counts
// with one ballot + popcount per 64 elements (exact integers), waves of a workgroup are added in wave order and
// the per-workgroup partials in index order: deterministic two-stage reduction, no atomics.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) classify_partial_kernel(const float* pred, const float* label, int64_t n, float th,
                                                               unsigned long long* partial) {
  unsigned long long tp = 0, fp = 0, fn = 0;         // wave-uniform running counts
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < n;
    const bool p = in && pred[i] > th, l = in && label[i] > th;
    tp += __popcll(__ballot(p && l));
    fp += __popcll(__ballot(p && !l));
    fn += __popcll(__ballot(!p && l));
  }
  __shared__ unsigned long long sh[4][3];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[w][0] = tp; sh[w][1] = fp; sh[w][2] = fn; }
  __syncthreads();
  if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}
__global__ void classify_final_kernel(const unsigned long long* partial, int nblocks, double* sums3) {
  if (threadIdx.x < 3) {
    unsigned long long a = 0;
    for (int i = 0; i < nblocks; ++i) a += partial[i * 3 + threadIdx.x];
    sums3[threadIdx.x] = (double)a;
  }
}
// the three maps themselves (get_confusion_matrix returns tensors)
__global__ void __launch_bounds__(256) confusion_kernel(const float* pred, const float* label, int64_t n, float th, float* tp,
                                                        float* fp, float* fn) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float p = pred[i] > th ? 1.f : 0.f, l = label[i] > th ? 1.f : 0.f;
    tp[i] = p * l;
    fp[i] = p * (1.f - l);
    fn[i] = (1.f - p) * l;
  }
}

// ---------------------------------------------------------------------------
// Focal loss (loss.py:83-93).  Per element, in float32 like the reference's tensors:
//   pt_1 = clip(y_true == 1 ? y_pred : 1, 1e-3, .999),  pt_0 = clip(y_true == 0 ? y_pred : 0, 1e-3, .999)
//   term = alpha * (1 - pt_1)^gamma * log(pt_1) + (1 - alpha) * pt_0^gamma * log(1 - pt_0);  loss = -sum(term)
// (the clipped constants of the "other" class contribute their small fixed terms, as in the reference).
// Sum: per-lane doubles, 64-lane butterfly (wave reduction), waves in order, workgroup partials in order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float focal_term(float yp, float yt, float gamma, float alpha) {
  float pt1 = yt == 1.f ? yp : 1.f, pt0 = yt == 0.f ? yp : 0.f;
  pt1 = fminf(fmaxf(pt1, 1e-3f), .999f);
  pt0 = fminf(fmaxf(pt0, 1e-3f), .999f);
  const float a = alpha * powf(1.f - pt1, gamma) * logf(pt1);
  const float b = (1.f - alpha) * powf(pt0, gamma) * logf(1.f - pt0);
  return a + b;
}
__global__ void __launch_bounds__(256) focal_partial_kernel(const float* yp, const float* yt, int64_t n, float gamma, float alpha,
                                                            double* partial) {
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    s += (double)focal_term(yp[i], yt[i], gamma, alpha);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __shared__ double sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// 64 lanes: lane l adds the partials l, l + 64, ... (ascending), lane 0 then adds the 64 stripes in lane order — the same
// fixed-order striping as bce_final_kernel (a serial chain of nblocks / 64 + 64 additions instead of nblocks)
__global__ void focal_final_kernel(const double* partial, int nblocks, double* out) {
  __shared__ double sh[64];
  double a = 0;
  for (int i = threadIdx.x; i < nblocks; i += 64) a += partial[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
    for (int j = 0; j < 64; ++j) t += sh[j];
    out[0] = -t;
  }
}
// d loss / d y_pred * gscale; the clip passes no gradient outside [1e-3, .999] (tf.clip_by_value)
__global__ void __launch_bounds__(256) focal_bwd_kernel(const float* yp, const float* yt, int64_t n, float gamma, float alpha,
                                                        float gscale, float* dyp) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float p = yp[i], t = yt[i];
    float g = 0.f;
    if (p >= 1e-3f && p <= .999f) {
      if (t == 1.f) g = -alpha * (powf(1.f - p, gamma) / p - gamma * powf(1.f - p, gamma - 1.f) * logf(p));
      else if (t == 0.f) g = -(1.f - alpha) * (gamma * powf(p, gamma - 1.f) * logf(1.f - p) - powf(p, gamma) / (1.f - p));
    }
    dyp[i] = g * gscale;
  }
}

__global__ void voxelize_kernel(const int32_t* p, int64_t n, int cs, float* cubes, int B) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = p[i * 4 + 0], x = p[i * 4 + 1], y = p[i * 4 + 2], z = p[i * 4 + 3];
  if (c < 0 || c >= B || (unsigned)x >= (unsigned)cs || (unsigned)y >= (unsigned)cs || (unsigned)z >= (unsigned)cs) return;
  cubes[(((int64_t)c * cs + x) * cs + y) * cs + z] = 1.0f;
}

// the same from the partition's own outputs: global coordinates + sorted-cube index per point (-1 = dropped), for the
// cubes [lo, hi) only; x mod cs is taken here, so the host builds no per-point records
__global__ void voxelize_points_kernel(const int32_t* pts, const int32_t* cube_of_point, int64_t n, int cs, int lo, int hi, float* cubes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = cube_of_point[i];
  if (c < lo || c >= hi) return;
  int v[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { const int m = pts[i * 3 + a] % cs; v[a] = m < 0 ? m + cs : m; }   // numpy's non-negative remainder
  cubes[(((int64_t)(c - lo) * cs + v[0]) * cs + v[1]) * cs + v[2]] = 1.0f;
}

// ---------------------------------------------------------------------------
// D1 (point-to-point) geometry distortion, as MPEG pc_error computes it for the reference's eval
// (myutils/pc_error_wrapper.py:26-75, eval.py:194-207): mean over A of the squared distance to the nearest
// point of B.  Clouds are voxelised (integer coordinates < res), so B becomes an occupancy bit set and every point of A
// searches it with nearest_d2 (voxel_grid.h).  Exact.
// ---------------------------------------------------------------------------
constexpr int kD1Blocks = 1024;

__global__ void __launch_bounds__(256) d1_partial_kernel(const int32_t* pa, int64_t na, const unsigned* bits, int res,
                                                         double* partial, unsigned* max_d2) {
  __shared__ double sh[256];
  double acc = 0.0;
  unsigned worst = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na; i += (int64_t)gridDim.x * 256) {
    const int x = pa[i * 3], y = pa[i * 3 + 1], z = pa[i * 3 + 2];
    const unsigned best = nearest_d2(bits, res, x, y, z);
    acc += (double)best;
    worst = max(worst, best);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
  atomicMax(max_d2, worst);               // integer atomic: order-free
}

__global__ void d1_final_kernel(const double* partial, int nb, int64_t na, const unsigned* max_d2, double* out2) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += partial[i];
    out2[0] = s / (double)na;             // mse  (pc_error "mse1 (p2point)")
    out2[1] = (double)*max_d2;            // squared Hausdorff distance ("h. 1(p2point)")
  }
}

// ---------------------------------------------------------------------------
// D2 (point-to-plane) distortion of MPEG pc_error 0.13.4 with its defaults (neighborsProc = 1, averageNormals = 1)
// as the reference's eval calls it (myutils/pc_error_wrapper.py:46-51, `-n normal1`).  Behaviour pinned by
// black-box runs of the prebuilt pc_error_d (tools/make_golden.py, tests/golden/pc_error_d2.npz):
//   * T(p) = ALL points of the target cloud at the minimal distance from p (ties are common on a voxel grid);
//   * the target's normals, when it has none (the decoded cloud), are transferred from the source: normal(q) =
//     plain mean (not renormalised) of normal(p) over every p with q in T(p);
//   * p2plane(p) = mean over q in T(p) of ((p - q) . normal(q))^2;  mse = mean over p, "h." = max over p.
// The target cloud is given sorted by linear key so that a grid cell maps to its point index by binary search.
// Normal sums use 64-bit fixed-point integer atomics (exact, order-free), so the result is reproducible.
// ---------------------------------------------------------------------------
// calls f(j, ex, ey, ez) for every target point j at squared distance `best` from (x, y, z); e = p - q
template <typename F>
__device__ __forceinline__ void for_each_tied(const unsigned* bits, const int64_t* keys, int64_t nq, int res, int x, int y, int z,
                                              unsigned best, F f) {
  for_each_at_distance(bits, res, x, y, z, best, [&](int dx, int dy, int qz) {
    f(find_sorted_key(keys, nq, cell_of(res, x + dx, y + dy, qz)), -dx, -dy, z - qz);     // present: the bit is set
  });
}

constexpr double kNormalFix = 1099511627776.0;      // 2^40 fixed point for the normal sums

__global__ void __launch_bounds__(256) d2_transfer_kernel(const int32_t* p, int64_t np, const float* normals_p, const unsigned* bits,
                                                          const int64_t* qkeys, int64_t nq, int res, long long* sums, int* counts) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
    const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    const unsigned best = nearest_d2(bits, res, x, y, z);
    long long fx[3];
    for (int c = 0; c < 3; ++c) fx[c] = (long long)llrint((double)normals_p[i * 3 + c] * kNormalFix);
    for_each_tied(bits, qkeys, nq, res, x, y, z, best, [&](int64_t j, int, int, int) {
      for (int c = 0; c < 3; ++c) atomicAdd(reinterpret_cast<unsigned long long*>(&sums[j * 3 + c]), (unsigned long long)fx[c]);
      atomicAdd(&counts[j], 1);
    });
  }
}

__global__ void d2_normals_final_kernel(const long long* sums, const int* counts, int64_t nq, float* normals_q) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  const int c = counts[j];
  for (int k = 0; k < 3; ++k) normals_q[j * 3 + k] = c ? (float)((double)sums[j * 3 + k] / kNormalFix / (double)c) : 0.f;
}

__global__ void __launch_bounds__(256) d2_partial_kernel(const int32_t* p, int64_t np, const unsigned* bits, const int64_t* qkeys,
                                                         int64_t nq, const float* normals_q, int res, double* partial,
                                                         double* partial_max) {
  __shared__ double sh[256], shm[256];
  double acc = 0.0, worst = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
    const int x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    const unsigned best = nearest_d2(bits, res, x, y, z);
    double s = 0.0;
    int cnt = 0;
    for_each_tied(bits, qkeys, nq, res, x, y, z, best, [&](int64_t j, int ex, int ey, int ez) {
      const double d = (double)ex * (double)normals_q[j * 3] + (double)ey * (double)normals_q[j * 3 + 1] +
                       (double)ez * (double)normals_q[j * 3 + 2];
      s += d * d;
      ++cnt;
    });
    const double e = cnt ? s / (double)cnt : 0.0;
    acc += e;
    worst = fmax(worst, e);
  }
  sh[threadIdx.x] = acc;
  shm[threadIdx.x] = worst;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh[threadIdx.x] += sh[threadIdx.x + o];
      shm[threadIdx.x] = fmax(shm[threadIdx.x], shm[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partial[blockIdx.x] = sh[0]; partial_max[blockIdx.x] = shm[0]; }
}

__global__ void d2_final_kernel(const double* partial, const double* partial_max, int nb, int64_t np, double* out2) {
  if (threadIdx.x == 0) {
    double s = 0.0, m = 0.0;
    for (int i = 0; i < nb; ++i) { s += partial[i]; m = fmax(m, partial_max[i]); }
    out2[0] = s / (double)np;
    out2[1] = m;
  }
}

}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_topk_workspace_bytes(int B, int64_t vox) { (void)B; (void)vox; return 0; }

int pcgc_topk_threshold(const float* x, const int32_t* k_per_cube, int B, int64_t vox, int use_fixed, float fixed_thres,
                        float* thresholds, uint8_t* mask, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  (void)workspace; (void)workspace_bytes;
  if (B == 0) return 0;
  PCGC_REQUIRE(x && thresholds && (use_fixed || k_per_cube) && B >= 0 && vox > 0 && vox < ((int64_t)1 << 32),
               "pcgc_topk_threshold: bad arguments");
  if (B == 0) return 0;
  hipLaunchKernelGGL(topk_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, k_per_cube, vox, use_fixed, fixed_thres,
                     thresholds, mask);
  return launch_ok("topk_kernel");
}

size_t pcgc_bce_workspace_bytes(int64_t n) { (void)n; return kBceBlocks * 4 * sizeof(double); }

int pcgc_bce_sums(const float* pred, const float* label, int64_t n, double* sums4, void* workspace, size_t workspace_bytes,
                  pcgc_stream_t stream) {
  PCGC_REQUIRE(pred && label && sums4 && workspace && workspace_bytes >= pcgc_bce_workspace_bytes(n), "pcgc_bce_sums: bad arguments");
  int blocks = (int)((n + 255) / 256);
  if (blocks > kBceBlocks) blocks = kBceBlocks;
  if (blocks < 1) blocks = 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bce_partial_kernel, dim3(blocks), dim3(256), 0, s, pred, label, n, (double*)workspace);
  hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks, sums4);
  return launch_ok("bce kernels");
}

size_t pcgc_classify_workspace_bytes(void) { return kBceBlocks * 3 * sizeof(unsigned long long); }

int pcgc_classify_sums(const float* pred, const float* label, int64_t n, float th, double* sums3, void* workspace,
                       size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(pred && label && sums3 && workspace && n >= 0 && workspace_bytes >= pcgc_classify_workspace_bytes(),
               "pcgc_classify_sums: bad arguments");
  int blocks = (int)((n + 255) / 256);
  if (blocks > kBceBlocks) blocks = kBceBlocks;
  if (blocks < 1) blocks = 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(classify_partial_kernel, dim3(blocks), dim3(256), 0, s, pred, label, n, th, (unsigned long long*)workspace);
  hipLaunchKernelGGL(classify_final_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)workspace, blocks, sums3);
  return launch_ok("classify kernels");
}

int pcgc_confusion_matrix(const float* pred, const float* label, int64_t n, float th, float* tp, float* fp, float* fn,
                          pcgc_stream_t stream) {
  PCGC_REQUIRE(n >= 0 && (n == 0 || (pred && label && tp && fp && fn)), "pcgc_confusion_matrix: bad arguments");
  if (n == 0) return 0;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, label, n, th, tp, fp, fn);
  return launch_ok("confusion_kernel");
}

size_t pcgc_focal_workspace_bytes(void) { return kBceBlocks * sizeof(double); }

int pcgc_focal_loss(const float* y_pred, const float* y_true, int64_t n, float gamma, float alpha, double* loss, void* workspace,
                    size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(y_pred && y_true && loss && workspace && n >= 0 && workspace_bytes >= pcgc_focal_workspace_bytes(),
               "pcgc_focal_loss: bad arguments");
  int blocks = (int)((n + 255) / 256);
  if (blocks > kBceBlocks) blocks = kBceBlocks;
  if (blocks < 1) blocks = 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(focal_partial_kernel, dim3(blocks), dim3(256), 0, s, y_pred, y_true, n, gamma, alpha, (double*)workspace);
  hipLaunchKernelGGL(focal_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks, loss);
  return launch_ok("focal kernels");
}

int pcgc_focal_loss_bwd(const float* y_pred, const float* y_true, int64_t n, float gamma, float alpha, float grad_scale,
                        float* dy_pred, pcgc_stream_t stream) {
  PCGC_REQUIRE(n >= 0 && (n == 0 || (y_pred && y_true && dy_pred)), "pcgc_focal_loss_bwd: bad arguments");
  if (n == 0) return 0;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(focal_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y_pred, y_true, n, gamma, alpha,
                     grad_scale, dy_pred);
  return launch_ok("focal_bwd_kernel");
}

size_t pcgc_d1_workspace_bytes(int res) {
  const size_t words = ((size_t)res * res * res + 31) / 32;
  return words * sizeof(unsigned) + kD1Blocks * sizeof(double) + 256;
}

int pcgc_d1_mse(const int32_t* pa, int64_t na, const int32_t* pb, int64_t nb, int res, double* out2, void* workspace,
                size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(pa && pb && out2 && workspace && na > 0 && nb > 0 && res > 0 && res <= 4096, "pcgc_d1_mse: bad arguments");
  PCGC_REQUIRE(workspace_bytes >= pcgc_d1_workspace_bytes(res), "pcgc_d1_mse: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t words = ((size_t)res * res * res + 31) / 32;
  unsigned* bits = reinterpret_cast<unsigned*>(workspace);
  double* partial = reinterpret_cast<double*>(bits + ((words + 1) & ~(size_t)1));
  unsigned* maxd = reinterpret_cast<unsigned*>(partial + kD1Blocks);
  PCGC_CHECK_HIP(hipMemsetAsync(bits, 0, words * sizeof(unsigned), s));
  PCGC_CHECK_HIP(hipMemsetAsync(maxd, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(bits_from_points_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, pb, nb, res, bits);
  int blocks = (int)((na + 255) / 256);
  if (blocks > kD1Blocks) blocks = kD1Blocks;
  hipLaunchKernelGGL(d1_partial_kernel, dim3(blocks), dim3(256), 0, s, pa, na, bits, res, partial, maxd);
  hipLaunchKernelGGL(d1_final_kernel, dim3(1), dim3(64), 0, s, partial, blocks, na, maxd, out2);
  return launch_ok("d1 kernels");
}

size_t pcgc_d2_workspace_bytes(int res, int64_t nq) {
  const size_t words = ((size_t)res * res * res + 31) / 32;
  return ((words + 1) & ~(size_t)1) * sizeof(unsigned) + (size_t)nq * (3 * sizeof(long long) + sizeof(int)) + 16 +
         2 * kD1Blocks * sizeof(double) + 256;
}

static int d2_layout(int res, int64_t nq, const int64_t* qkeys, void* workspace, size_t workspace_bytes, hipStream_t s, unsigned** bits,
                     long long** sums, int** counts, double** partial) {
  PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_d2_workspace_bytes(res, nq), "pcgc_d2: workspace too small");
  const size_t words = ((size_t)res * res * res + 31) / 32;
  *bits = reinterpret_cast<unsigned*>(workspace);
  *sums = reinterpret_cast<long long*>(*bits + ((words + 1) & ~(size_t)1));
  *counts = reinterpret_cast<int*>(*sums + 3 * nq);
  *partial = reinterpret_cast<double*>(reinterpret_cast<char*>(*counts) + (((size_t)nq * sizeof(int) + 15) & ~(size_t)15));
  PCGC_CHECK_HIP(hipMemsetAsync(*bits, 0, words * sizeof(unsigned), s));
  hipLaunchKernelGGL(bits_from_keys_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, qkeys, nq,
                     (int64_t)res * res * res, *bits);
  return 0;
}

int pcgc_d2_transfer_normals(const int32_t* p, int64_t np, const float* normals_p, const int64_t* qkeys, int64_t nq, int res,
                             float* normals_q, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(p && normals_p && qkeys && normals_q && np > 0 && nq > 0 && res > 0 && res <= 4096, "pcgc_d2_transfer_normals: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  unsigned* bits; long long* sums; int* counts; double* partial;
  int rc = d2_layout(res, nq, qkeys, workspace, workspace_bytes, s, &bits, &sums, &counts, &partial);
  if (rc) return rc;
  PCGC_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)nq * (3 * sizeof(long long) + sizeof(int)), s));
  int blocks = (int)std::min<int64_t>((np + 255) / 256, 4096);
  hipLaunchKernelGGL(d2_transfer_kernel, dim3(blocks), dim3(256), 0, s, p, np, normals_p, bits, qkeys, nq, res, sums, counts);
  hipLaunchKernelGGL(d2_normals_final_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, sums, counts, nq, normals_q);
  return launch_ok("d2 normal transfer kernels");
}

int pcgc_d2_mse(const int32_t* p, int64_t np, const int64_t* qkeys, int64_t nq, const float* normals_q, int res, double* out2,
                void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(p && qkeys && normals_q && out2 && np > 0 && nq > 0 && res > 0 && res <= 4096, "pcgc_d2_mse: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  unsigned* bits; long long* sums; int* counts; double* partial;
  int rc = d2_layout(res, nq, qkeys, workspace, workspace_bytes, s, &bits, &sums, &counts, &partial);
  if (rc) return rc;
  int blocks = (int)std::min<int64_t>((np + 255) / 256, kD1Blocks);
  hipLaunchKernelGGL(d2_partial_kernel, dim3(blocks), dim3(256), 0, s, p, np, bits, qkeys, nq, normals_q, res, partial, partial + kD1Blocks);
  hipLaunchKernelGGL(d2_final_kernel, dim3(1), dim3(64), 0, s, partial, partial + kD1Blocks, blocks, np, out2);
  return launch_ok("d2 kernels");
}

int pcgc_voxelize(const int32_t* cube_xyz, int64_t n, int cube_size, float* cubes, int B, pcgc_stream_t stream) {
  PCGC_REQUIRE(cubes && (n == 0 || cube_xyz) && cube_size > 0 && B >= 0, "pcgc_voxelize: bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(voxelize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cube_xyz, n,
                     cube_size, cubes, B);
  return launch_ok("voxelize_kernel");
}

int pcgc_voxelize_points(const int32_t* points, const int32_t* cube_of_point, int64_t n, int cube_size, int cube_lo, int cube_hi,
                         float* cubes, pcgc_stream_t stream) {
  PCGC_REQUIRE(cubes && (n == 0 || (points && cube_of_point)) && cube_size > 0 && cube_lo >= 0 && cube_hi >= cube_lo,
               "pcgc_voxelize_points: bad arguments");
  if (n == 0 || cube_hi == cube_lo) return 0;
  hipLaunchKernelGGL(voxelize_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points,
                     cube_of_point, n, cube_size, cube_lo, cube_hi, cubes);
  return launch_ok("voxelize_points_kernel");
}

}  // extern "C"
