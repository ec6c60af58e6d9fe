// Host-side plan of one pcgc_net_forward call (net.hip): where every region of the caller's workspace lies, which part of
// a table belongs to a chunk and a launch, where the empty-cube responses lie in the net's blob.  pcgc_net_workspace_bytes
// SIZES the workspace with the plan pcgc_net_forward CARVES it with.  Plain C++17, no HIP: tests/net_plan_check.cpp.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/pcgc.h"
#include "workspace.h"            // Arena: the workspace plan and the weight blob

namespace pcgc {

constexpr int kSkipLaunches = 8;                // conv_in, A / BC of the three C = 16 blocks, down_1
constexpr int kSkipLaunchesMid = 6;             // A / BC of the three C = 32 blocks (32^3 stage of the analysis)
constexpr int kSegMaxChunk = 48;                // cubes per launch of the segment form (slot codes hold the cube above bit 10)
constexpr int kSegLaunches = 7;                 // conv_in, kernel A / BC of the three C = 16 blocks
constexpr int kHyperChunk = 256;                // cubes per launch of the hyper encoder / decoder

// Launch numbers inside a chunk's tables: the 64^3 stage (tile orders of kSkipLaunches launches; the slot lists of the
// segment form hold the first kSegLaunches of them) and the 32^3 stage.  Block i = 0 .. 2.
namespace l64 { constexpr int conv_in = 0, down_1 = 7; constexpr int A(int i) { return 1 + 2 * i; } constexpr int BC(int i) { return 2 + 2 * i; } }
namespace l32 { constexpr int A(int i) { return 2 * i; } constexpr int BC(int i) { return 2 * i + 1; } }
static_assert(l64::down_1 == l64::BC(2) + 1 && l64::down_1 + 1 == kSkipLaunches && l64::BC(2) + 1 == kSegLaunches &&
              l32::BC(2) + 1 == kSkipLaunchesMid, "the launch numbers fill the tables");
// per cube and launch: tile-order entries at 64^3 / 32^3, virtual-row words, slots, bytes of the slots' "not written" table
constexpr size_t kTiles64 = 512, kTiles32 = 256, kVirtWords = 64, kSlots = 1024, kSegVirtBytes = 256;

// The analysis' responses to an EMPTY cube, in floats from the start of the net's blob of them: an all-zero input cube, the
// 64^3 set e_in | e_t[3] | e_o[3] (conv_in's output, tensor1_1 | tensor2_1 and the output of each C = 16 block, Q4), the
// 32^3 set (down_1 and the C = 32 blocks), then the TileCfg tables.
struct StageOffsets { size_t first = 0, t[3] = {}, o[3] = {}, end = 0; };      // the stage input's response, then per block
constexpr StageOffsets stage_offsets(size_t at, size_t vox, size_t c) {
  StageOffsets s;
  s.first = at; at += vox * c;
  for (int i = 0; i < 3; ++i) { s.t[i] = at; at += vox * (c / 2); }
  for (int i = 0; i < 3; ++i) { s.o[i] = at; at += vox * c; }
  s.end = at;
  return s;
}
struct EmptyLayout {
  StageOffsets s64 = stage_offsets(64 * 64 * 64, 64 * 64 * 64, 16), s32 = stage_offsets(s64.end, 32 * 32 * 32, 32);
  size_t cfg = s32.end, total = cfg + 256;
  constexpr size_t copy_floats() const { return s64.end - s64.first; }     // what the slot kernels and down_1 may read
};
inline constexpr EmptyLayout kEmpty{};

// PCGC_SKIP_EMPTY: 0 = compute every tile; 1 = empty tiles are not written at all, readers take the empty-cube response for
// them (only the stage's last launch materialises its empty tiles, for down_1); 2 = every launch copies its empty tiles (all tensors
// complete); 3 = as 1, with the three C = 16 blocks on SLOTS of 8 planes x 2 rows x 16 voxels (vrn_seg.hip) — the default.
struct Chunks { int big, mid, small; };                    // cubes per launch at D, D/2, D/4; asked.big == 0: the defaults
inline Chunks chunk_plan(int kind, int mode, bool responses, Chunks asked) {
  const bool skipping = kind == PCGC_NET_ANALYSIS && responses && mode != 0;
  Chunks c{8, 64, 256};
  // the analysis' 64^3 stage with empty-space skipping computes about half of its tiles: 16 cubes per launch keep two
  // heavy waves on every SIMD (one wave alone runs at 0.6 of the pair's rate; measured 8 / 12 / 16 / 24: DESIGN.md §3)
  if (skipping) c.big = 16;
  // the blocks on slots compute a fifth to a third of them: about 36 cubes per launch put two waves on every SIMD once
  // (1 024 slots per cube, four per wave, 2 048 wave places; measured 16 / 32 / 40: profiles/r06_vB_seg_chunks.txt)
  if (skipping && mode == 3) c.big = 40;
  if (asked.big > 0) c = asked;
  if (skipping && mode == 3 && c.big > kSegMaxChunk) c.big = kSegMaxChunk;       // the slot lists' limit
  return c;
}
// 64^3 chunks of equal size (103 cubes: 7 x 15 or 14 instead of 6 x 16 + 7): with empty-space skipping a launch takes
// as long as its fullest SIMD, so a short last chunk costs as much as a full one, and chunks just over the size that
// fills every wave slot once pay a second round (profiles/r04_vC_skip_launches.txt)
inline int equal_chunk(int nb, int chunk) { const int k = (nb + chunk - 1) / chunk; return (nb + k - 1) / k; }

struct Span { size_t at = 0, bytes = 0; };                // bytes == 0: this net has no such region
enum Region {
  R_S2, R_S3, R_WORK,                                      // stage boundaries kept per super chunk; one chunk's tensor + VRN scratch
  R_ROWOCC, R_VIRT, R_ORDER, R_ORDER_MID, R_N_HEAVY, R_N_HEAVY_MID,       // RowSkip tables (launch_tile_order)
  R_OCC64, R_SEG_SLOTS, R_SEG_COUNTS, R_SEG_VIRT, R_EMPTY_COPY,           // the segment form's (launch_seg_order)
  R_F1, R_F2, R_F3, R_COUNT                                // hyper encoder / decoder activations
};
// One table of the chunk of n cubes that starts at cube c0 of its super chunk: `launches` parts of n * per_cube elements,
// launch c's at + c * step bytes — the strides tile_order_kernel (common.h: launch_tile_order) and seg_order_kernel
// (vrn_seg.hip) document.  A table of counts has one element per (chunk, launch): c0 = the chunk's index, n = per_cube = 1.
template <class T>
struct Table {
  size_t at = 0, step = 0;
  Table() = default;
  Table(const Span& region, int launches, size_t per_cube, int c0, int n)
      : at(region.at + (size_t)c0 * launches * per_cube * sizeof(T)), step((size_t)n * per_cube * sizeof(T)) {}
  size_t launch(int c) const { return at + (size_t)c * step; }
  const T* in(const char* ws, int c) const { return reinterpret_cast<const T*>(ws + launch(c)); }     // ws = the workspace's aligned base
};
struct ChunkView {
  int A0;                                                  // launch number of block 0's kernel A: block i's A = A0 + 2i, its BC one more
  Table<unsigned> order, n_heavy, slots, counts;
  Table<unsigned long long> virt; Table<unsigned char> seg_virt;
};

struct NetPlan {
  int mode = 0;
  bool responses = false, skip_mid = true, copy_empty = false;     // the net has empty-cube responses; PCGC_SKIP_MID; PCGC_SEG_COPY_EMPTY
  Chunks ch{0, 0, 0}; int SC = 0;                          // SC: cubes per super chunk (autoencoder) or per chunk (hyper nets)
  size_t V = 0, s2_cube = 0, s3_cube = 0;                  // voxels at full resolution, floats per cube of S2 / S3
  Span r[R_COUNT]; size_t total = 0;

  // the tables of the 64^3 chunk of n cubes that starts at cube c0 of its super chunk, k = its index among the chunks
  ChunkView chunk64(int c0, int n, int k) const {
    return {l64::A(0), {r[R_ORDER], kSkipLaunches, kTiles64, c0, n}, {r[R_N_HEAVY], kSkipLaunches, 1, k, 1},
            {r[R_SEG_SLOTS], kSegLaunches, kSlots, c0, n}, {r[R_SEG_COUNTS], kSegLaunches, 1, k, 1},
            {r[R_VIRT], kSkipLaunches, kVirtWords, c0, n}, {r[R_SEG_VIRT], kSegLaunches, kSegVirtBytes, c0, n}};
  }
  ChunkView chunk32(int c0, int n, int k) const {          // ... of the 32^3 chunk: tile orders and counts only
    return {l32::A(0), {r[R_ORDER_MID], kSkipLaunchesMid, kTiles32, c0, n}, {r[R_N_HEAVY_MID], kSkipLaunchesMid, 1, k, 1}, {}, {}, {}, {}};
  }
};

inline NetPlan plan_net(int kind, int B, int D, Chunks asked, int mode, bool responses) {
  NetPlan p; Arena a;
  p.mode = mode; p.responses = responses;
  // alignment by what reads a region: 16 bytes for float tensors, a cache line for tables of 64-bit words, 256 for the copy
  auto take = [&](Region r, size_t count, size_t elem, size_t align) { p.r[r] = Span{a.take(count * elem, align), count * elem}; };
  auto least = [](int x, int y) { return (size_t)std::min(x, y); };
  const size_t d3 = (size_t)D * D * D;
  if (kind == PCGC_NET_ANALYSIS || kind == PCGC_NET_SYNTHESIS) {
    const bool ana = kind == PCGC_NET_ANALYSIS;
    const Chunks c = p.ch = chunk_plan(kind, mode, responses, asked);
    const size_t V = p.V = ana ? d3 : d3 * 64;
    const size_t SC = p.SC = std::min(B, std::max({c.big, c.mid, c.small}));
    p.s2_cube = (V / 8) * 32;
    p.s3_cube = ana ? (V / 64) * 64 : 0;                     // synthesis keeps no 64^3 stage buffer
    const size_t work = std::max({least(B, c.big) * V * 16, least(B, c.mid) * p.s2_cube, least(B, c.small) * (V / 64) * 64});
    take(R_S2, SC * p.s2_cube, 4, 16);
    take(R_S3, SC * p.s3_cube, 4, 16);
    take(R_WORK, work + (work / 4) * 3, 4, 16);             // one activation tensor (blocks run in place) + VRN scratch
    // RowSkip tables per cube of the super chunk; the heavy-tile counts per (chunk, launch), at most one chunk per cube
    take(R_ROWOCC, SC * 64, 8, 64);
    take(R_VIRT, SC * kSkipLaunches * kVirtWords, 8, 64);
    take(R_ORDER, SC * kSkipLaunches * kTiles64, 4, 4);
    take(R_ORDER_MID, SC * kSkipLaunchesMid * kTiles32, 4, 4);
    take(R_N_HEAVY, SC * kSkipLaunches, 4, 4);
    take(R_N_HEAVY_MID, SC * kSkipLaunchesMid, 4, 4);
    if (ana && D == 64 && responses) {
      // the segment form: 64 x 64 voxel-occupancy words, slot lists, a count per launch, "not written" bytes; per call the
      // responses the slot kernels and down_1 may read, copied here when the net's own copy is out of the window's reach
      take(R_OCC64, SC * 64 * 64, 8, 64);
      take(R_SEG_SLOTS, SC * kSegLaunches * kSlots, 4, 4);
      take(R_SEG_COUNTS, SC * kSegLaunches, 4, 4);
      take(R_SEG_VIRT, SC * kSegLaunches * kSegVirtBytes, 1, 1);
      take(R_EMPTY_COPY, kEmpty.copy_floats(), 4, 256);
    }
  } else if (kind == PCGC_NET_HYPER_ENCODER || kind == PCGC_NET_HYPER_DECODER) {
    const size_t n = p.SC = std::min(B, kHyperChunk);
    const bool enc = kind == PCGC_NET_HYPER_ENCODER;
    take(R_F1, n * d3 * 16, 4, 16);
    take(R_F2, n * d3 * (enc ? 2 : 8 * 16), 4, 16);
    if (!enc) take(R_F3, n * d3 * 8 * 32, 4, 16);
  }
  p.total = a.end;
  return p;
}

}  // namespace pcgc
