// Stand-alone check of csrc/net_plan.h (the workspace plan of pcgc_net_forward): g++ -std=c++17 -O1 -Wall -Werror, no GPU.
// tests/test_net_plan.py builds and runs it.  Exit status 0 = every combination holds.
#include <cstdio>

#include "../pcgcv1_amd/csrc/net_plan.h"

using namespace pcgc;

static long g_failures = 0;
static char g_case[160];
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (++g_failures <= 20) {                             \
        std::printf("FAIL %s: %s: ", g_case, #cond);        \
        std::printf(__VA_ARGS__);                           \
        std::printf("\n");                                  \
      }                                                     \
    }                                                       \
  } while (0)

// ORACLE: the workspace size the hand-written ws_floats() of net.hip gave before the plan existed (commit 042b3e5),
// restated term by term, + the 256 bytes for aligning the caller's pointer.  c = the resolved chunk sizes.
static size_t parent_workspace_bytes(int kind, int B, int D, Chunks c, bool responses) {
  auto imin = [](int a, int b) { return a < b ? a : b; };
  const size_t kSkipFloatsPerCube = 128 + (size_t)kSkipLaunches * 512 + (size_t)kSkipLaunches * 128 + (size_t)kSkipLaunchesMid * 256 +
                                    kSkipLaunches + kSkipLaunchesMid;
  const size_t kSegFloatsPerCube = 2 * 4096 + (size_t)kSegLaunches * 1024 + (size_t)kSegLaunches * 64 + kSegLaunches;
  const size_t kSegEmptyFloats = (size_t)64 * 64 * 64 * (16 + 3 * 8 + 3 * 16);
  const size_t d3 = (size_t)D * D * D;
  size_t floats = 0;
  if (kind == PCGC_NET_ANALYSIS || kind == PCGC_NET_SYNTHESIS) {
    const bool ana = kind == PCGC_NET_ANALYSIS;
    const size_t V = ana ? d3 : d3 * 64;
    const int widest = c.big > c.mid ? (c.big > c.small ? c.big : c.small) : (c.mid > c.small ? c.mid : c.small);
    const size_t SC = (size_t)imin(B, widest);
    const size_t s2 = SC * (V / 8) * 32, s3 = SC * (ana ? (V / 64) * 64 : 0);
    const size_t wb = (size_t)imin(B, c.big) * V * 16, wm = (size_t)imin(B, c.mid) * (V / 8) * 32, wsm = (size_t)imin(B, c.small) * (V / 64) * 64;
    size_t work = wb > wm ? wb : wm;
    if (wsm > work) work = wsm;
    floats = s2 + s3 + work + (work / 4) * 3 + SC * kSkipFloatsPerCube + 64 + (ana && D == 64 && responses ? SC * kSegFloatsPerCube + kSegEmptyFloats + 256 : 0);
  } else if (kind == PCGC_NET_HYPER_ENCODER) {
    floats = (size_t)imin(B, 256) * (d3 * 16 + d3 * 2);
  } else {
    floats = (size_t)imin(B, 256) * (d3 * 16 + d3 * 8 * 16 + d3 * 8 * 32);
  }
  return floats * sizeof(float) + 256;
}

// ORACLE: the chunk sizes chunk_plan() of net.hip resolved at the same commit, restated
static Chunks parent_chunks(int kind, int mode, bool responses, Chunks asked) {
  Chunks c{8, 64, 256};
  if (kind == PCGC_NET_ANALYSIS && responses && mode != 0) c.big = 16;
  if (kind == PCGC_NET_ANALYSIS && responses && mode == 3) c.big = 40;
  if (asked.big > 0) c = asked;
  if (kind == PCGC_NET_ANALYSIS && responses && mode == 3 && c.big > 48) c.big = 48;
  return c;
}

// launches 0 .. count - 1 of table t lie back to back inside region s and end at or before `next` (the same table of the
// next chunk, or the region's end)
template <class T>
static void check_table(const char* what, const Table<T>& t, int count, const Span& s, size_t next) {
  CHECK(s.bytes != 0, "%s: the region is not laid out", what);
  CHECK(t.at >= s.at, "%s starts at %zu, region at %zu", what, t.at, s.at);
  for (int c = 0; c < count; ++c) CHECK(t.launch(c) + t.step == t.launch(c + 1), "%s launch %d", what, c);
  CHECK(t.launch(count) <= next && next <= s.at + s.bytes, "%s ends at %zu, its neighbour starts at %zu, the region ends at %zu", what,
        t.launch(count), next, s.at + s.bytes);
}

static void check_plan(int kind, int B, int D, Chunks asked, int mode, bool responses) {
  std::snprintf(g_case, sizeof(g_case), "kind %d B %d D %d chunks %d,%d,%d mode %d responses %d", kind, B, D, asked.big, asked.mid, asked.small,
                mode, (int)responses);
  const NetPlan p = plan_net(kind, B, D, asked, mode, responses);
  const bool ana = kind == PCGC_NET_ANALYSIS, autoenc = ana || kind == PCGC_NET_SYNTHESIS;
  // alignment, order, disjointness, total
  size_t end = 0;
  for (int r = 0; r < R_COUNT; ++r) {
    const Span& s = p.r[r];
    if (s.bytes == 0) continue;
    const bool words = r == R_ROWOCC || r == R_VIRT || r == R_OCC64;
    const bool floats = r == R_S2 || r == R_S3 || r == R_WORK || r == R_F1 || r == R_F2 || r == R_F3;
    const size_t need = r == R_EMPTY_COPY ? 256 : words ? 64 : floats ? 16 : r == R_SEG_VIRT ? 1 : 4;
    CHECK(s.at % need == 0, "region %d at %zu is not aligned to %zu", r, s.at, need);
    CHECK(s.at >= end, "region %d at %zu overlaps its predecessor, which ends at %zu", r, s.at, end);
    end = s.at + s.bytes;
  }
  CHECK(end == p.total, "last end %zu, total %zu", end, p.total);
  const bool segment_tables = ana && D == 64 && responses;
  CHECK((p.r[R_EMPTY_COPY].bytes != 0) == segment_tables && (p.r[R_SEG_SLOTS].bytes != 0) == segment_tables, "segment regions");
  if (segment_tables) CHECK(p.r[R_EMPTY_COPY].bytes == (size_t)64 * 64 * 64 * (16 + 3 * 8 + 3 * 16) * 4, "copy of %zu bytes", p.r[R_EMPTY_COPY].bytes);
  // against the oracle: never larger, and smaller only by the removed slack
  const Chunks pc = parent_chunks(kind, mode, responses, asked);
  if (autoenc) CHECK(p.ch.big == pc.big && p.ch.mid == pc.mid && p.ch.small == pc.small, "chunks %d,%d,%d, the parent's %d,%d,%d", p.ch.big, p.ch.mid, p.ch.small, pc.big, pc.mid, pc.small);
  const size_t parent = parent_workspace_bytes(kind, B, D, pc, responses), mine = p.total + 256;
  CHECK(mine <= parent && parent - mine <= 1280, "workspace of %zu bytes, the parent's %zu", mine, parent);
  if (!autoenc) return;
  {
    // ORACLE: the offsets the pointer arithmetic of forward_autoencoder() gave at the same commit, restated: the tensors back to
    // back, the RowSkip tables from the next 64-byte boundary on, the segment form's from the next one, the copy at a 256-byte one
    auto up = [](size_t x, size_t a) { return (x + a - 1) / a * a; };
    const size_t SC = p.SC, s3 = SC * p.s2_cube * 4, work = s3 + SC * p.s3_cube * 4, rowocc = up(work + p.r[R_WORK].bytes, 64);
    const size_t virt = rowocc + SC * 64 * 8, order = virt + SC * kSkipLaunches * 64 * 8, order_mid = order + SC * kSkipLaunches * 512 * 4;
    const size_t n_heavy = order_mid + SC * kSkipLaunchesMid * 256 * 4, n_heavy_mid = n_heavy + SC * kSkipLaunches * 4;
    const size_t occ64 = up(n_heavy_mid + SC * kSkipLaunchesMid * 4, 64), slots = occ64 + SC * 4096 * 8, counts = slots + SC * kSegLaunches * 1024 * 4;
    const size_t seg_virt = counts + SC * kSegLaunches * 4, copy = up(seg_virt + SC * kSegLaunches * 256, 256);
    CHECK(p.r[R_S2].at == 0 && p.r[R_S3].at == s3 && p.r[R_WORK].at == work && p.r[R_ROWOCC].at == rowocc && p.r[R_VIRT].at == virt &&
          p.r[R_ORDER].at == order && p.r[R_ORDER_MID].at == order_mid && p.r[R_N_HEAVY].at == n_heavy && p.r[R_N_HEAVY_MID].at == n_heavy_mid,
          "tensors and RowSkip tables lie where the hand-written carve put them");
    if (segment_tables)
      CHECK(p.r[R_OCC64].at == occ64 && p.r[R_SEG_SLOTS].at == slots && p.r[R_SEG_COUNTS].at == counts && p.r[R_SEG_VIRT].at == seg_virt &&
            p.r[R_EMPTY_COPY].at == copy, "the segment form's tables lie where the hand-written carve put them");
  }
  if (ana && responses && mode == 3) CHECK(p.ch.big <= kSegMaxChunk, "mode-3 chunk of %d cubes", p.ch.big);
  // every chunk of every stage: its tables and tensors lie inside their regions and below the next chunk's
  const size_t F = sizeof(float), quarter = 4;
  for (int b0 = 0; b0 < B; b0 += p.SC) {
    const int nb = B - b0 < p.SC ? B - b0 : p.SC;
    const int big = equal_chunk(nb, p.ch.big);
    CHECK(big >= 1 && big <= p.ch.big, "equal chunks of %d cubes", big);
    for (int c0 = 0, k = 0; c0 < nb; c0 += big, ++k) {
      const int n = big < nb - c0 ? big : nb - c0;
      const bool last = c0 + n == nb;
      const ChunkView v = p.chunk64(c0, n, k), w = p.chunk64(c0 + n, 1, k + 1);
      auto next = [&](size_t theirs, Region r) { return last ? p.r[r].at + p.r[r].bytes : theirs; };
      check_table("order", v.order, kSkipLaunches, p.r[R_ORDER], next(w.order.at, R_ORDER));
      check_table("n_heavy", v.n_heavy, kSkipLaunches, p.r[R_N_HEAVY], next(w.n_heavy.at, R_N_HEAVY));
      check_table("virt", v.virt, kSkipLaunches, p.r[R_VIRT], next(w.virt.at, R_VIRT));
      CHECK(v.order.step == (size_t)n * 512 * 4 && v.virt.step == (size_t)n * 64 * 8, "strides of the tile orders");
      if (segment_tables) {
        check_table("slots", v.slots, kSegLaunches, p.r[R_SEG_SLOTS], next(w.slots.at, R_SEG_SLOTS));
        check_table("counts", v.counts, kSegLaunches, p.r[R_SEG_COUNTS], next(w.counts.at, R_SEG_COUNTS));
        check_table("seg_virt", v.seg_virt, kSegLaunches, p.r[R_SEG_VIRT], next(w.seg_virt.at, R_SEG_VIRT));
        CHECK(v.slots.step == (size_t)n * 1024 * 4 && v.seg_virt.step == (size_t)n * 256, "strides of the slot lists");
      }
      // the chunk's 16-channel tensor + three quarters of it as VRN scratch; its part of S2
      CHECK((size_t)n * p.V * 16 * F / quarter * 7 <= p.r[R_WORK].bytes, "64^3 chunk of %d cubes in the work region", n);
      CHECK((size_t)(c0 + n) * p.s2_cube * F <= p.r[R_S2].bytes, "64^3 chunk in S2");
    }
    for (int c0 = 0, k = 0; c0 < nb; c0 += p.ch.mid, ++k) {
      const int n = p.ch.mid < nb - c0 ? p.ch.mid : nb - c0;
      const bool last = c0 + n == nb;
      const ChunkView v = p.chunk32(c0, n, k), w = p.chunk32(c0 + n, 1, k + 1);
      check_table("order_mid", v.order, kSkipLaunchesMid, p.r[R_ORDER_MID], last ? p.r[R_ORDER_MID].at + p.r[R_ORDER_MID].bytes : w.order.at);
      check_table("n_heavy_mid", v.n_heavy, kSkipLaunchesMid, p.r[R_N_HEAVY_MID], last ? p.r[R_N_HEAVY_MID].at + p.r[R_N_HEAVY_MID].bytes : w.n_heavy.at);
      CHECK(v.order.step == (size_t)n * 256 * 4, "stride of the 32^3 tile orders");
      CHECK((size_t)n * p.s2_cube * F / quarter * 3 <= p.r[R_WORK].bytes && (size_t)(c0 + n) * p.s2_cube * F <= p.r[R_S2].bytes, "32^3 chunk of %d cubes", n);
    }
    for (int c0 = 0; c0 < nb; c0 += p.ch.small) {
      const int n = p.ch.small < nb - c0 ? p.ch.small : nb - c0;
      const size_t cube = (p.V / 64) * 64 * F;                // a 16^3 cube of 64 channels
      // analysis: in place on S3, scratch in work; synthesis: tensor + scratch in work
      CHECK((size_t)n * cube / quarter * (ana ? 3 : 7) <= p.r[R_WORK].bytes, "16^3 chunk of %d cubes in the work region", n);
      if (ana) CHECK((size_t)(c0 + n) * cube <= p.r[R_S3].bytes, "16^3 chunk in S3");
    }
  }
}

int main() {
  const int Bs[] = {1, 2, 7, 16, 17, 40, 41, 48, 49, 205, 256, 257, 300};
  const Chunks plans[] = {{0, 0, 0} /* default */, {2, 3, 5}, {3, 16, 32}, {8, 70, 70}, {48, 48, 48}, {128, 128, 128}};
  // input sizes: the one the codec runs (64^3 cubes: analysis 64, latents 16, hyper latents 8) and a small one
  const int Ds[4][2] = {{64, 16}, {16, 4}, {16, 2}, {8, 1}};
  long n = 0;
  for (int kind = PCGC_NET_ANALYSIS; kind <= PCGC_NET_HYPER_DECODER; ++kind)
    for (int D : Ds[kind])
      for (int B : Bs)
        for (int mode = 0; mode <= 3; ++mode)
          for (int responses = 0; responses <= 1; ++responses)
            for (const Chunks& c : plans) {
              check_plan(kind, B, D, c, mode, responses != 0);
              ++n;
            }
  // the empty-cube responses: both sets back to back, the copy = the 64^3 set without the all-zero input
  const EmptyLayout& el = kEmpty;
  std::snprintf(g_case, sizeof(g_case), "empty_layout");
  const size_t V = 64 * 64 * 64;
  CHECK(el.s64.first == V && el.s64.t[0] == V * 17 && el.s64.o[0] == V * 41 && el.s64.o[2] + V * 16 == el.s32.first, "64^3 set");
  CHECK(el.copy_floats() == V * (16 + 3 * 8 + 3 * 16) && el.cfg == V * 89 + (V / 8) * (32 + 3 * 16 + 3 * 32) && el.total == el.cfg + 256, "sizes");
  std::printf("%ld plans checked, %ld failures\n", n, g_failures);
  return g_failures ? 1 : 0;
}
