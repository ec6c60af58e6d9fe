// Colour rate control (gfx950): what colorcodec.encode_colors_target needs beyond the codec's own kernels (raht.hip).
//   rate_sweep_kernel  prices up to 32 candidate quantiser steps in one pass over the coefficients: per (step, subband, channel)
//                      the sum of min(|q|, 2048) and per (step, subband) the largest |q| — the two numbers from which the host
//                      rebuilds every table of a real encode at that step, and with them the bytes it would write.
//   requantize_kernel  rint(coef / step) * step: quantise and dequantise in one go, for the closed-loop PSNR probe.
//   sse6_kernel        the six second moments of the difference of two uint8 colourings.
// DESIGN.md §7d states the rule; tests/_color_rc_ref.py is its definition in numpy.  Every sum is taken in integers (wave
// reduction, LDS partials, 64-bit atomics), so the results are exact and do not depend on the order of the additions; the file is
// built with -ffp-contract=off like raht.hip, and the quantiser's expression is raht.hip's, a division included.
#include "common.h"

namespace pcgc {
namespace {

constexpr int kBins = 37;                        // subbands 0 .. 35 and the DC, as raht.hip
constexpr int kThreads = 256;
constexpr int kMaxSteps = 32;
constexpr unsigned int kAbsCap = 2048u;          // AMAX_CAP + 1: what pcgc_raht_abs_sums counts an escaped value as
constexpr int kSseRows = 8;                      // rows per thread of sse6_kernel

struct SweepSteps { double s[kMaxSteps]; };      // by value in the kernel arguments: no upload, no device buffer to keep alive

unsigned blocks_for(int64_t n, int per = kThreads) { return (unsigned)((n + per - 1) / per); }

// pcgc_raht_quantize's expression (raht.hip: quantize_kernel)
__device__ __forceinline__ int quantise(double v, double step) {
  return (int)fmin(fmax(rint(v / step), -2147483647.0), 2147483647.0);
}

// The rows come in subband order, so a wave almost always holds one subband: it then adds its 64 values up with lane shuffles
// (the three channels' sums share one 64-bit word, 21 bits each: 64 x 2048 < 2^21) and makes one LDS atomic per channel and
// step; a wave that straddles two subbands falls back to one atomic per lane.  part holds at most 256 x 2048 per entry.
__global__ void __launch_bounds__(kThreads) rate_sweep_kernel(const double* coef, const int32_t* order, const int32_t* subband, int64_t n,
                                                              SweepSteps steps, int n_steps, unsigned long long* sums, int32_t* max_abs) {
  __shared__ unsigned int part[kMaxSteps * kBins * 3];
  __shared__ int mx[kMaxSteps * kBins];
  for (int i = threadIdx.x; i < n_steps * kBins * 3; i += kThreads) part[i] = 0;
  for (int i = threadIdx.x; i < n_steps * kBins; i += kThreads) mx[i] = 0;
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = k < n;
  int l = -1;
  double v[3] = {0.0, 0.0, 0.0};
  if (valid) {
    const int64_t j = order[k];
    l = min(max(subband[j], 0), kBins - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = coef[j * 3 + c];
  }
  const unsigned long long live = __ballot(valid);
  if (live) {                                                           // wave-uniform
    const int lref = __shfl(l, __ffsll((long long)live) - 1);
    const bool uniform = __all(!valid || l == lref);
    for (int i = 0; i < n_steps; ++i) {
      const double step = steps.s[i];
      unsigned int a[3];
      int top = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int q = quantise(v[c], step);
        const unsigned int u = q < 0 ? 0u - (unsigned int)q : (unsigned int)q;
        top = max(top, (int)u);
        a[c] = min(u, kAbsCap);
      }
      if (uniform) {
        unsigned long long w = (unsigned long long)a[0] | ((unsigned long long)a[1] << 21) | ((unsigned long long)a[2] << 42);
        for (int off = 32; off > 0; off >>= 1) {
          w += __shfl_down(w, off);
          top = max(top, __shfl_down(top, off));
        }
        if (lane == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const unsigned int s = (unsigned int)(w >> (21 * c)) & 0x1FFFFFu;
            if (s) atomicAdd(&part[(i * kBins + lref) * 3 + c], s);
          }
          if (top) atomicMax(&mx[i * kBins + lref], top);
        }
      } else if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (a[c]) atomicAdd(&part[(i * kBins + l) * 3 + c], a[c]);
        if (top) atomicMax(&mx[i * kBins + l], top);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_steps * kBins * 3; i += kThreads)
    if (part[i]) atomicAdd(&sums[i], (unsigned long long)part[i]);
  for (int i = threadIdx.x; i < n_steps * kBins; i += kThreads)
    if (mx[i] > 0) atomicMax(&max_abs[i], mx[i]);
}

// n = 3 M values; the int32 in between is pcgc_raht_quantize's q, the product pcgc_raht_dequantize's
__global__ void __launch_bounds__(kThreads) requantize_kernel(const double* coef, int64_t n, double step, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  out[i] = (double)quantise(coef[i], step) * step;
}

// a thread takes kSseRows rows (a term is at most 255^2, a block's sum at most 2048 x 255^2 < 2^31), the wave adds up with lane
// shuffles, the block in LDS, the grid with 64-bit atomics (two's complement: the mixed sums may be negative)
__global__ void __launch_bounds__(kThreads) sse6_kernel(const uint8_t* a, const uint8_t* b, int64_t m, unsigned long long* out) {
  __shared__ int part[6];
  if (threadIdx.x < 6) part[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * (kThreads * kSseRows) + threadIdx.x;
  int acc[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < kSseRows; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    if (i < m) {
      const int dr = (int)a[i * 3] - (int)b[i * 3], dg = (int)a[i * 3 + 1] - (int)b[i * 3 + 1], db = (int)a[i * 3 + 2] - (int)b[i * 3 + 2];
      acc[0] += dr * dr; acc[1] += dg * dg; acc[2] += db * db;
      acc[3] += dr * dg; acc[4] += dr * db; acc[5] += dg * db;
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int v = acc[c];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&part[c], v);
  }
  __syncthreads();
  if (threadIdx.x < 6 && part[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)(long long)part[threadIdx.x]);
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

int pcgc_raht_rate_sweep(const double* coef, const int32_t* order, const int32_t* subband, int64_t m, int64_t k_raw, const double* steps,
                         int n_steps, int64_t* abs_sums, int32_t* max_abs, pcgc_stream_t stream) {
  PCGC_REQUIRE(steps && abs_sums && max_abs && m > 0 && m <= 0x7FFFFFFF && k_raw >= 0 && k_raw <= m && (k_raw == 0 || (coef && order && subband)),
               "pcgc_raht_rate_sweep: bad arguments");
  PCGC_REQUIRE(n_steps >= 1 && n_steps <= kMaxSteps, "pcgc_raht_rate_sweep: %d steps, one call prices 1 .. %d", n_steps, kMaxSteps);
  SweepSteps st = {};
  for (int i = 0; i < n_steps; ++i) {
    PCGC_REQUIRE(steps[i] > 0.0 && steps[i] <= 1.7976931348623157e308, "pcgc_raht_rate_sweep: step %d is not a positive finite number", i);
    st.s[i] = steps[i];
  }
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemsetAsync(abs_sums, 0, (size_t)n_steps * kBins * 3 * sizeof(int64_t), s));
  PCGC_CHECK_HIP(hipMemsetAsync(max_abs, 0, (size_t)n_steps * kBins * sizeof(int32_t), s));
  if (k_raw == 0) return 0;
  hipLaunchKernelGGL(rate_sweep_kernel, dim3(blocks_for(k_raw)), dim3(kThreads), 0, s, coef, order, subband, k_raw, st, n_steps,
                     reinterpret_cast<unsigned long long*>(abs_sums), max_abs);
  return launch_ok("raht rate sweep kernel");
}

int pcgc_raht_requantize(const double* coef, int64_t m, double step, double* out, pcgc_stream_t stream) {
  PCGC_REQUIRE(coef && out && m > 0 && m <= 0x7FFFFFFF && step > 0.0 && step <= 1.7976931348623157e308, "pcgc_raht_requantize: bad arguments");
  PCGC_REQUIRE(out + 3 * m <= coef || coef + 3 * m <= out, "pcgc_raht_requantize: out overlaps coef");
  hipLaunchKernelGGL(requantize_kernel, dim3(blocks_for(3 * m)), dim3(kThreads), 0, (hipStream_t)stream, coef, 3 * m, step, out);
  return launch_ok("raht requantise kernel");
}

int pcgc_color_sse6(const uint8_t* rgb_a, const uint8_t* rgb_b, int64_t m, int64_t* out, pcgc_stream_t stream) {
  PCGC_REQUIRE(rgb_a && rgb_b && out && m > 0 && m <= 0x7FFFFFFF, "pcgc_color_sse6: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  PCGC_CHECK_HIP(hipMemsetAsync(out, 0, 6 * sizeof(int64_t), s));
  hipLaunchKernelGGL(sse6_kernel, dim3(blocks_for(m, kThreads * kSseRows)), dim3(kThreads), 0, s, rgb_a, rgb_b, m,
                     reinterpret_cast<unsigned long long*>(out));
  return launch_ok("colour sse6 kernel");
}

}  // extern "C"
