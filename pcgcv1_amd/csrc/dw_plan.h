// Host-side description of the weight-gradient dispatch (train_dw.hip): which kernel instantiation a call takes, with which
// grid, and whether the training plan's deferred mode may batch it.  launch_conv_dw_tile / _s2 / _pair choose here, then
// launch; callers size their partial buffers with the same functions.  Plain C++17, no HIP: tests/dw_plan_check.cpp.
#pragma once
#include <algorithm>
#include <cstddef>

namespace pcgc {

constexpr int kDwGroups = 512;     // persistent workgroups of a tiled kernel (x2 per CU) = partial sums per weight
constexpr int kDwChunks = 128;     // voxel chunks of the generic kernel (train.hip conv_dw_partial_kernel)
constexpr int kDwPartials = std::max(kDwGroups, kDwChunks);     // workspace slots per weight, whichever kernel runs

// One value per kernel instantiation train_dw.hip can launch (name: Cin per chunk x Cout); kGeneric = none of them.
enum class DwKernel : int {
  kGeneric,
  kOne_16x4, kOne_4x8,                                   // conv_dw_1x1_kernel<CIN, COUT>
  kMfma4_4, kMfma4_8,                                    // conv_dw_mfma_4xn_kernel<COUT>
  kMfma16_4, kMfma16_8, kMfma16Pair_4, kMfma16Pair_8,    // conv_dw_mfma_16xn_kernel<COUT, PAIR>
  kMfma_8x16, kMfma_16x16, kMfma_16x32, kMfma_16x64,     // conv_dw_mfma_kernel<COUT, 1, CIN>
  kMfmaS2_16x16, kMfmaS2_16x32, kMfmaS2_16x64,           // conv_dw_mfma_kernel<COUT, 2>
  kSlide_4x4, kSlide_4x8, kSlide_8x8,                    // conv_dw_slide_kernel<CIN, COUT, WSEG>
  kEdge_16x1, kEdge_1x16,                                // conv_dw_mfma_edge_kernel<MODE>
  kTile1_16x8, kTile1_8x16, kTile1_16x16, kTile1_16x32,  // conv_dw_tile1_kernel<CIN, COUT>
  kCount
};
inline const char* dw_kernel_name(DwKernel k) {
  constexpr const char* names[] = {
      "generic", "conv_dw_1x1_kernel<16, 4>", "conv_dw_1x1_kernel<4, 8>", "conv_dw_mfma_4xn_kernel<4>", "conv_dw_mfma_4xn_kernel<8>",
      "conv_dw_mfma_16xn_kernel<4, false>", "conv_dw_mfma_16xn_kernel<8, false>", "conv_dw_mfma_16xn_kernel<4, true>", "conv_dw_mfma_16xn_kernel<8, true>",
      "conv_dw_mfma_kernel<16, 1, 8>", "conv_dw_mfma_kernel<16, 1, 16>", "conv_dw_mfma_kernel<32, 1, 16>", "conv_dw_mfma_kernel<64, 1, 16>",
      "conv_dw_mfma_kernel<16, 2, 16>", "conv_dw_mfma_kernel<32, 2, 16>", "conv_dw_mfma_kernel<64, 2, 16>",
      "conv_dw_slide_kernel<4, 4, 4>", "conv_dw_slide_kernel<4, 8, 4>", "conv_dw_slide_kernel<8, 8, 8>",
      "conv_dw_mfma_edge_kernel<0>", "conv_dw_mfma_edge_kernel<1>",
      "conv_dw_tile1_kernel<16, 8>", "conv_dw_tile1_kernel<8, 16>", "conv_dw_tile1_kernel<16, 16>", "conv_dw_tile1_kernel<16, 32>"};
  static_assert(sizeof(names) / sizeof(names[0]) == (size_t)DwKernel::kCount, "one name per kernel");
  return names[(int)k];
}

// Workgroups of a tiled launch: one 4 x 4 x 16 tile each for stride 1, two 2 x 2 x 16 (coarse) tiles each for stride 2, at
// most kDwGroups.  Every workgroup writes a partial sum of the WHOLE filter gradient, which the final reduction reads again:
// for down_2 / up_1 (27 x 32 x 64 weights) on 8 cubes that is 512 tiles -> 113 MB written and read per layer with one tile per
// workgroup.  Two tiles each: the step 8.54 -> 8.47 ms (four: the same).  The stride-1 layers of the 16^3 stage, 128 tiles:
// 8.53 with two, 8.63 with four, so one; 256 instead of 512 workgroups for the 1 024 tiles of the 32^3 stage: 8.36 against 8.34.
inline int conv_dw_tile_groups(int B, int D) { return std::min(B * (D / 4) * (D / 4) * (D / 16), kDwGroups); }
inline int conv_dw_tile_groups_s2(int B, int D) {          // D = coarse grid
  return std::min((B * (D / 2) * (D / 2) * (D / 16) + 1) / 2, kDwGroups);
}

// kernel == kGeneric && !refused: no tiled kernel, the caller runs the generic one.  refused: an operand is in the Q4 layout
// and the kernel of this shape (or the generic one) would read the wrong voxels.  Otherwise grid = (groups, chunks) and the
// partial sums are [groups][taps * Cin * Cout (+ Cout bias sums)].
struct DwChoice {
  DwKernel kernel = DwKernel::kGeneric;
  bool refused = false;
  int groups = 0, chunks = 0;
  bool batchable = false;            // the deferred mode may run several such calls as the jobs of one launch (grid.z)
};

// Operand layouts a kernel reads, as bits 1 << (x_q4 + 2 * dz_q4).  A 4-channel x is the same bytes in both layouts but only
// its NDHWC flag is accepted; a 1-channel operand has no Q4 form and its flag is ignored when the other operand is Q4.
constexpr unsigned kDwNdhwc = 1, kDwQ4x = 2, kDwQ4dz = 4, kDwQ4both = 8;

// The stride-1 ladder, first match wins.  A row takes ksize and Cout exactly, Cin == cin or (any_multiple) Cin = n * cin as
// n channel chunks (grid.y), and only_D != 0 restricts it to that cube size.  Rows overlap in one place only: 4 -> 4 / 8 at
// 64^3 goes to the whole-row MFMA kernels (tiles of 4 x 4 x 64), every other D to the sliding VALU kernels below them.
struct DwRule { DwKernel kernel; int ksize, cin; bool any_multiple; int cout, only_D; unsigned layouts; bool batchable; };
constexpr DwRule kDwRules[] = {
    // 1^3 with at most 64 (ci, co) pairs: register-resident sums, reads x and dz once
    {DwKernel::kOne_16x4, 1, 16, false, 4, 0, kDwNdhwc, false},
    {DwKernel::kOne_4x8, 1, 4, false, 8, 0, kDwNdhwc | kDwQ4dz, false},
    // 3^3, narrow operands: taps fill the idle MFMA rows / columns
    {DwKernel::kMfma4_4, 3, 4, false, 4, 64, kDwNdhwc, false},
    {DwKernel::kMfma4_8, 3, 4, false, 8, 64, kDwNdhwc | kDwQ4dz, false},
    {DwKernel::kMfma16_4, 3, 16, true, 4, 0, kDwNdhwc, false},
    {DwKernel::kMfma16_8, 3, 16, true, 8, 0, kDwNdhwc, false},
    {DwKernel::kMfma_8x16, 3, 8, false, 16, 0, kDwNdhwc, false},
    {DwKernel::kSlide_4x4, 3, 4, false, 4, 0, kDwNdhwc, false},
    {DwKernel::kSlide_4x8, 3, 4, false, 8, 0, kDwNdhwc, false},
    {DwKernel::kSlide_8x8, 3, 8, false, 8, 0, kDwNdhwc, false},      // (MFMA with half of the columns idle: 25 against 23 us)
    // 3^3, 16 x 16 and wider: one tap per MFMA row block
    {DwKernel::kMfma_16x16, 3, 16, true, 16, 0, kDwNdhwc, true},
    {DwKernel::kMfma_16x32, 3, 16, true, 32, 0, kDwNdhwc, true},
    {DwKernel::kMfma_16x64, 3, 16, true, 64, 0, kDwNdhwc, true},
    // 3^3, one operand with a single channel: the taps fill its side of the matrix
    {DwKernel::kEdge_16x1, 3, 16, false, 1, 0, kDwNdhwc | kDwQ4x | kDwQ4both, false},
    {DwKernel::kEdge_1x16, 3, 1, false, 16, 0, kDwNdhwc | kDwQ4dz | kDwQ4both, false},
    // 1^3 with more pairs than registers: the LDS-tiled VALU kernel
    {DwKernel::kTile1_16x8, 1, 16, true, 8, 0, kDwNdhwc, false},
    {DwKernel::kTile1_8x16, 1, 8, false, 16, 0, kDwNdhwc, false},
    {DwKernel::kTile1_16x16, 1, 16, true, 16, 0, kDwNdhwc, true},
    {DwKernel::kTile1_16x32, 1, 16, true, 32, 0, kDwNdhwc, true},
};

// Stride-1 layer (ksize 1 or 3), x and dz [B, D^3, Cin / Cout]
inline DwChoice dw_choose(int ksize, int Cin, int Cout, int D, int B, int x_q4, int dz_q4) {
  DwChoice c;
  if (D % 16) return c;
  const unsigned layout = 1u << ((x_q4 ? 1 : 0) + (dz_q4 ? 2 : 0));
  for (const DwRule& r : kDwRules) {
    if (ksize != r.ksize || Cout != r.cout || (r.only_D && D != r.only_D)) continue;
    if (r.any_multiple ? (Cin < r.cin || Cin % r.cin) : Cin != r.cin) continue;
    // (the 1^3 kernel on a Q4 dz keeps a thread on one w: the row length must divide the 256 voxels a workgroup walks)
    if (!(r.layouts & layout) || (dz_q4 && r.kernel == DwKernel::kOne_4x8 && 256 % D)) break;
    c.kernel = r.kernel;
    c.groups = conv_dw_tile_groups(B, D);
    c.chunks = Cin / r.cin;
    c.batchable = r.batchable;
    return c;
  }
  c.refused = x_q4 || dz_q4;
  return c;
}

// Stride-2 pair, 3x3x3: fine = the operand on the (2 D)^3 grid with Ca channels (x of a stride-2 conv, dz of a transposed
// conv), coarse = the one on the D^3 grid with Cb channels; only the fine operand may be Q4.
inline DwChoice dw_choose_s2(int Ca, int Cb, int D, int B, int fine_q4) {
  DwChoice c;
  if (D % 16) return c;
  if (Ca >= 16 && Ca % 16 == 0 && (Cb == 16 || Cb == 32 || Cb == 64)) {
    c.kernel = Cb == 16 ? DwKernel::kMfmaS2_16x16 : (Cb == 32 ? DwKernel::kMfmaS2_16x32 : DwKernel::kMfmaS2_16x64);
    c.groups = conv_dw_tile_groups_s2(B, D);
    c.chunks = Ca / 16;
    return c;
  }
  c.refused = fine_q4 != 0;
  return c;
}

// conv1_1 (3x3x3) and conv2_1 (1x1x1) of a VRN block, both Cin -> Cout on the same input (NDHWC or Q4), in one pass over it
inline DwChoice dw_choose_pair(int Cin, int Cout, int D, int B) {
  DwChoice c;
  if (D % 16 || Cin < 16 || Cin % 16 || (Cout != 4 && Cout != 8)) return c;
  c.kernel = Cout == 4 ? DwKernel::kMfma16Pair_4 : DwKernel::kMfma16Pair_8;
  c.groups = conv_dw_tile_groups(B, D);
  c.chunks = Cin / 16;
  return c;
}
inline bool conv_dw_pair_supported(int D, int Cin, int Cout) { return dw_choose_pair(Cin, Cout, D, 1).kernel != DwKernel::kGeneric; }

// floats of partial sums one layer's weight gradient needs at (B, D): *bias_floats more for the bias-only partials
inline size_t bwd_weight_partial_floats(int B, int D, int Cin, int Cout, int ksize, int stride, int transposed, size_t* bias_floats) {
  const size_t wn = (size_t)ksize * ksize * ksize * Cin * Cout;
  const int groups = transposed ? conv_dw_tile_groups_s2(B, D) : (stride == 2 ? conv_dw_tile_groups_s2(B, D / 2) : conv_dw_tile_groups(B, D));
  *bias_floats = (size_t)1024 * Cout;
  return (size_t)std::max(groups, kDwChunks) * (wn + Cout);
}

}  // namespace pcgc
