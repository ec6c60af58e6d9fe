// Device helpers shared by the row kernels on v_mfma_f32_4x4x1_16B_f32 (vrn_row.hip / vrn_seg.hip: 64^3 / C = 16,
// vrn_row32.hip: 32^3 / C = 32, vrn_row16.hip: 16^3 / C = 64): the 16-block MFMA with A broadcast (cbsz = 4, abid = k), DPP
// lane shifts, raw buffer loads / stores whose out-of-range offsets read zeros / drop the store, the 3^3 tap walk of the 64^3
// kernels and the role rotation of the plane loops.  See vrn_row.hip for the mapping.
#pragma once
#include <type_traits>
#include "common.h"

namespace pcgc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// hipcc 7.2 lowers __builtin_amdgcn_raw_buffer_load_b128 to a ONE-dword load; bind the intrinsics directly
__device__ f32x4 raw_load4(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ float raw_load1(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");
__device__ void raw_store4(f32x4 v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4f32");
__device__ void raw_store1i(int v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.i32");

__device__ __forceinline__ i32x4 make_rsrc(const void* p, unsigned bytes) {
  const unsigned long long a = (unsigned long long)p;
  i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
  r[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu));
  r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  r[3] = 0x00020000;
  return r;
}
// Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8), each with a private L2: give every XCD a
// CONTIGUOUS range of tiles, so that the halo rows neighbouring tiles share are fetched into one L2 once (speed only).
__device__ __forceinline__ int xcd_contiguous(int bid, int nblk) {
  return (nblk & 7) ? bid : (bid & 7) * (nblk >> 3) + (bid >> 3);
}
constexpr int kOOB = 0x7ffff000;   // byte offset past any cube: the buffer load returns 0

template <int ABID>
__device__ __forceinline__ f32x4 mf(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, ABID, 0);
}
// abid is a compile-time constant after unrolling; the switch folds away
__device__ __forceinline__ f32x4 mfa(int abid, float a, float b, f32x4 c) {
  switch (abid) {
    case 0: return mf<0>(a, b, c);
    case 1: return mf<1>(a, b, c);
    case 2: return mf<2>(a, b, c);
    case 3: return mf<3>(a, b, c);
    case 4: return mf<4>(a, b, c);
    case 5: return mf<5>(a, b, c);
    case 6: return mf<6>(a, b, c);
    case 7: return mf<7>(a, b, c);
    case 8: return mf<8>(a, b, c);
    case 9: return mf<9>(a, b, c);
    case 10: return mf<10>(a, b, c);
    case 11: return mf<11>(a, b, c);
    case 12: return mf<12>(a, b, c);
    case 13: return mf<13>(a, b, c);
    case 14: return mf<14>(a, b, c);
    default: return mf<15>(a, b, c);
  }
}

// The first MFMA of an accumulator: C = bias / zero, D = registers of their own.  The empty asm keeps a, b and d alive
// together, so D is never allocated on top of a dying operand.  History: in round 2 fresh accumulators came out wrong in
// lanes 12..15 of each row of 16 when a second wave shared the SIMD (cubes 4..7 of an 8-cube launch, run to run
// different) and this constraint made it go away; it was read as "a 4x4x1 MFMA must not have D over B".  Round 3 tested
// that directly (tools/exp/exp_mfma_overlap.hip: D over A, B or both, every position / abid / occupancy, 324 variants):
// no mismatch — the overlap is harmless.  What the constraint really changed was WHERE the new accumulator landed: without
// it the allocator reused the registers of the rows just handed to a 128-bit buffer_store with a register soffset, the one
// store form the compiler does not protect against an overwrite of its data (see rsrc_at in vrn_row.hip; tools/check_isa.py
// refuses that form in the object code).  Kept: it costs nothing and keeps the allocation away from in-flight store data.
// Validated with hipcc 7.2.26015 / clang 22.0.0git (roc-7.2.0); tests: test_every_row_kernel_is_slot_invariant_and_repeatable.
__device__ __forceinline__ f32x4 mfa_new(int abid, float a, float b, f32x4 c) {
  f32x4 d = mfa(abid, a, b, c);
  asm("" : "+v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ float shr1(float v) {   // lane i <- lane i-1, lane 0 <- 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float shl1(float v) {   // lane i <- lane i+1, lane 63 <- 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
  return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
}
__device__ __forceinline__ float comp(const f32x4& v, int c) { return v[c]; }
// on a lambda handed to one of the templates below: its body belongs into the unrolled nest whatever the inliner's cost model says
// (left to that model, loops around it stay rolled: -Wpass-failed)
#define PCGC_INLINE __attribute__((always_inline))

// ---------------------------------------------------------------------------------------------------------------
// The 3^3 tap walk of the 64^3 kernels (vrn_row.hip, vrn_seg.hip), written once.  A wave holds TH rows of three output
// planes in three accumulator sets and reads input planes one at a time: input plane p feeds the output planes p - 1, p,
// p + 1 (kd = 2, 1, 0), held in sets P0, P1, P2 (vJ: set J takes part — wave-uniform, ONE branch per set), and its row r (of
// TH + 2: one halo row on either side) feeds output row jr = r - kh.  For NC channels of that plane the walk calls
//   mac(set, jr, r, kw, tap, born, c)   for every (c, r, kh, kw) that lands on one of the TH output rows, then
//   rider(j, c)                         once per (output plane j = 0, 1, 2, channel): a 1^3 layer riding in plane j's branch
// so every accumulator receives its contributions in the order (plane, channel, kh, kw), the planes coming from the kernel's
// plane loop.  tap = (kd * 3 + kh) * NKW + kw (NKW = 1: the site folds kw into its MFMA rows, deconv_out).  born (FRESH only):
// this is the first (channel, kh) that reaches accumulator row jr of set P2, the plane that gets its first contribution
// (kd = 0) in this step — with the site's own "first kw" test, the MFMA that takes the bias as its C operand (mfa_new)
// instead of the stale accumulator: no initialisation moves.
// Call it from a function under the kernel (a_quad, bc_channel12, a step's quad lambda).  Where the nest sits in the kernel's
// own body (conv_in, vrn16bc_bwd_row_kernel) it stays written out: the compiler optimises the walk with the site's closure on
// its own before it becomes part of the caller, and a kernel that never had a function there comes out with another schedule.
// ---------------------------------------------------------------------------------------------------------------
struct NoRider {
  __device__ __forceinline__ void operator()(int, int) const {}
};
template <int TH, int P0, int P1, int P2, bool FRESH = false, int NKW = 3, int NC = 1, class MAC, class RIDER = NoRider>
__device__ __forceinline__ void tap_walk(bool v0, bool v1, bool v2, MAC mac, RIDER rider = RIDER()) {
  const bool vj[3] = {v0, v1, v2};
  constexpr int P[3] = {P0, P1, P2};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int kd = 2 - j;                      // input plane p feeds output plane p + 1 - kd = p - 1 + j
    if (vj[j]) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int r = 0; r < TH + 2; ++r)
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            const int jr = r - kh;
            if (jr >= 0 && jr < TH) {
#pragma unroll
              for (int kw = 0; kw < NKW; ++kw) mac(P[j], jr, r, kw, (kd * 3 + kh) * NKW + kw, FRESH && c == 0 && j == 2 && kh == 0, c);
            }
          }
        rider(j, c);
      }
    }
  }
}

// The driver of a plane loop whose accumulator sets keep their registers: the ROLES rotate instead.  step(p, R0, R1, R2) runs
// for p = first, first + 1, ... while `p cmp bound` (cmp: < or <=), unrolled three times, with R0 / R1 / R2 = integral
// constants naming the set that plays the step's first / second / third role.  Forward (back = false; the 3^3 kernels: roles = output planes p - 1, p, p + 1) the set that
// was second becomes first; back = true (up2_row_kernel: roles = output planes 2p, 2p + 1, 2p + 2) the set that was third does.
// A macro, not a template: a function that takes the kernel's step closure is optimised on its own, with the three step
// bodies inlined into it and the kernel's registers behind pointers, BEFORE it becomes part of the kernel, and the kernels
// come out with other schedules and register allocations (tried by value, by reference, with constant bounds).
using I0 = std::integral_constant<int, 0>;
using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;
template <bool BACK, class FWD, class BWD>
using RotateRole = std::conditional_t<BACK, BWD, FWD>;
#define PCGC_ROTATE3(first, cmp, bound, step, back)                                                                      \
  _Pragma("unroll 1") for (int p_ = (first); p_ cmp (bound); p_ += 3) {                                                   \
    step(p_, I0{}, I1{}, I2{});                                                                                          \
    if (!(p_ + 1 cmp (bound))) break;                                                                                    \
    step(p_ + 1, RotateRole<back, I1, I2>{}, RotateRole<back, I2, I0>{}, RotateRole<back, I0, I1>{});                    \
    if (!(p_ + 2 cmp (bound))) break;                                                                                    \
    step(p_ + 2, RotateRole<back, I2, I1>{}, RotateRole<back, I0, I2>{}, RotateRole<back, I1, I0>{});                    \
  }

// ---------------------------------------------------------------------------------------------------------------
// Kernel BC of the C = 16 block at 64^3, one input channel ci of conv1_2 (4 -> 8; weights [27][4][8]: VGPR tap >> 1, abid =
// (tap & 1) * 8 + ci * 2 + half) / conv2_2 (4 -> 4; [27][4][4]: VGPR tap >> 2, abid = (tap & 3) * 4 + ci), for the row
// kernel and the segment kernel alike.  rows(r, ci, x0, xm, xp) is the site's shift source: channel ci of input row r and
// its kw = 0 / 2 neighbours (vrn_row.hip: wave shifts with zero fill, vrn_seg.hip: shifts inside a slot with edge values).
// P0, P1, P2: which of the three accumulator sets holds output plane p-1, p, p+1 in this step (PCGC_ROTATE3: the sets
// never move between registers).  FRESH: this call holds the first tap that reaches each accumulator of set P2 (tap_walk: born).
// ---------------------------------------------------------------------------------------------------------------
template <int TH, int P0, int P1, int P2, bool FRESH, class ROWS>
__device__ __forceinline__ void bc_channel12(f32x4 (&acc)[3][TH][2], const f32x4 (&bias)[2], const float (&W)[14], int ci, ROWS rows, bool v0,
                                             bool v1, bool v2) {
  float x0[TH + 2], xm[TH + 2], xp[TH + 2];
#pragma unroll
  for (int r = 0; r < TH + 2; ++r) rows(r, ci, x0[r], xm[r], xp[r]);
  tap_walk<TH, P0, P1, P2, FRESH>(v0, v1, v2, [&](int set, int jr, int r, int kw, int t, bool born, int) PCGC_INLINE {
    const float xv = kw == 0 ? xm[r] : (kw == 1 ? x0[r] : xp[r]);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const bool first = born && kw == 0;
      acc[set][jr][hf] = first ? mfa_new((t & 1) * 8 + ci * 2 + hf, W[t >> 1], xv, bias[hf])
                               : mfa((t & 1) * 8 + ci * 2 + hf, W[t >> 1], xv, acc[set][jr][hf]);
    }
  });
}
template <int TH, int P0, int P1, int P2, bool FRESH, class ROWS>
__device__ __forceinline__ void bc_channel22(f32x4 (&acc)[3][TH], const f32x4& bias, const float (&W)[7], int ci, ROWS rows, bool v0, bool v1,
                                             bool v2) {
  float x0[TH + 2], xm[TH + 2], xp[TH + 2];
#pragma unroll
  for (int r = 0; r < TH + 2; ++r) rows(r, ci, x0[r], xm[r], xp[r]);
  tap_walk<TH, P0, P1, P2, FRESH>(v0, v1, v2, [&](int set, int jr, int r, int kw, int t, bool born, int) PCGC_INLINE {
    const float xv = kw == 0 ? xm[r] : (kw == 1 ? x0[r] : xp[r]);
    const bool first = born && kw == 0;
    acc[set][jr] = first ? mfa_new((t & 3) * 4 + ci, W[t >> 2], xv, bias) : mfa((t & 3) * 4 + ci, W[t >> 2], xv, acc[set][jr]);
  });
}

// lds[i] = f(i) for i < N by 256 threads, the loads of 16 elements per thread in flight before their LDS writes (the
// plain `for (i = tid; ...) lds[i] = w[index(i)]` loop waits for every load in turn)
template <int N, class F>
__device__ __forceinline__ void stage_indexed(float* lds, F f) {
  constexpr int IT = (N + 255) / 256;
#pragma unroll
  for (int k0 = 0; k0 < IT; k0 += 16) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int i = (k0 + k) * 256 + threadIdx.x;
      v[k] = (k0 + k < IT && i < N) ? f(i) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int i = (k0 + k) * 256 + threadIdx.x;
      if (k0 + k < IT && i < N) lds[i] = v[k];
    }
  }
}

// N floats global -> LDS by 256 threads: every 16-byte load is issued before the first LDS write, so the copy costs one
// memory round trip instead of one per loop iteration
template <int N>
__device__ __forceinline__ void stage_image(float* lds, const float* __restrict__ g) {
  constexpr int IT = (N / 4 + 255) / 256;
  float4 v[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = (k * 256 + threadIdx.x) * 4;
    v[k] = i < N ? *reinterpret_cast<const float4*>(g + i) : float4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = (k * 256 + threadIdx.x) * 4;
    if (i < N) *reinterpret_cast<float4*>(lds + i) = v[k];
  }
}

// the same for a workgroup of T threads
template <int N, int T>
__device__ __forceinline__ void stage_image_t(float* lds, const float* __restrict__ g) {
  constexpr int IT = (N / 4 + T - 1) / T;
  float4 v[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = (k * T + threadIdx.x) * 4;
    v[k] = i < N ? *reinterpret_cast<const float4*>(g + i) : float4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = (k * T + threadIdx.x) * 4;
    if (i < N) *reinterpret_cast<float4*>(lds + i) = v[k];
  }
}

}  // namespace pcgc
