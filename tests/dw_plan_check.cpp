// Stand-alone check of csrc/dw_plan.h (the weight-gradient dispatch of train_dw.hip): g++ -std=c++17 -O1 -Wall -Werror, no GPU.
// tests/test_dw_plan.py builds it and runs it on a file of layer records taken from models/spec.py.  Exit status 0 = the
// chooser agrees with the ladder it replaced everywhere but on the printed exceptions, no layer is among them, every enum
// value is reachable and every partial buffer is large enough.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "../pcgcv1_amd/csrc/dw_plan.h"

using namespace pcgc;

static long g_failures = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      if (++g_failures <= 20) {                        \
        std::printf("FAIL %s: ", #cond);               \
        std::printf(__VA_ARGS__);                      \
        std::printf("\n");                             \
      }                                                \
    }                                                  \
  } while (0)

// ORACLE: launch_conv_dw_tile / launch_conv_dw_tile_s2 / conv_dw_pair_supported of train_dw.hip at commit 97cc34f, restated
// rung by rung with each of its eight environment knobs at its default (all kernels enabled, one tile per workgroup for
// stride 1, two for stride 2).  Kernels are named as that file instantiated them.
struct Old {
  std::string kernel = "generic";
  bool refused = false;
  int groups = 0, chunks = 0;
  bool batchable = false;
};
static std::string fmt(const char* f, int a, int b = 0, int c = 0, int d = 0) {
  char buf[96];
  std::snprintf(buf, sizeof buf, f, a, b, c, d);
  return buf;
}
static int old_groups(int B, int D) { const int n = B * (D / 4) * (D / 4) * (D / 16); return n < 512 ? n : 512; }
static int old_groups_s2(int B, int D) { const int n = (B * (D / 2) * (D / 2) * (D / 16) + 2 - 1) / 2; return n < 512 ? n : 512; }
static Old old_run_dw_mfma(int COUT, int STRIDE, int CIN, int Cin, int g, int x_q4) {      // run_dw_mfma<COUT, STRIDE, CIN>
  return Old{fmt("conv_dw_mfma_kernel<%d, %d, %d>", COUT, STRIDE, CIN), false, g, Cin / CIN, STRIDE == 1 && CIN == 16 && !x_q4};
}
static Old old_stride1(int ksize, int Cin, int Cout, int D, int B, int x_q4, int dz_q4) {
  if (D % 16) return Old{};
  const int g = old_groups(B, D);
  if (x_q4 || dz_q4) {
    if (ksize == 3 && Cin == 16 && Cout == 1 && x_q4) return Old{"conv_dw_mfma_edge_kernel<0>", false, g, 1, false};
    if (ksize == 3 && Cin == 1 && Cout == 16 && dz_q4) return Old{"conv_dw_mfma_edge_kernel<1>", false, g, 1, false};
    if (ksize == 3 && Cin == 4 && Cout == 8 && D == 64 && dz_q4 && !x_q4) return Old{"conv_dw_mfma_4xn_kernel<8>", false, g, 1, false};
    if (ksize == 1 && Cin == 4 && Cout == 8 && dz_q4 && !x_q4) {
      if (256 % D) return Old{"generic", true};
      return Old{"conv_dw_1x1_kernel<4, 8>", false, g, 1, false};
    }
    return Old{"generic", true};
  }
  if (ksize == 1 && ((Cin == 16 && Cout == 4) || (Cin == 4 && Cout == 8)))
    return Old{Cin == 16 ? "conv_dw_1x1_kernel<16, 4>" : "conv_dw_1x1_kernel<4, 8>", false, g, 1, false};
  if (ksize == 3 && Cin == 4 && (Cout == 4 || Cout == 8) && D == 64) return Old{fmt("conv_dw_mfma_4xn_kernel<%d>", Cout), false, g, 1, false};
  if (ksize == 3 && Cin % 16 == 0 && (Cout == 4 || Cout == 8)) return Old{fmt("conv_dw_mfma_16xn_kernel<%d, false>", Cout), false, g, Cin / 16, false};
  if (ksize == 3 && Cin == 8) {
    if (Cout == 16) return old_run_dw_mfma(16, 1, 8, Cin, g, 0);
  }
  // SLIDE(ck, co, wseg)
  static const int slide[8][3] = {{4, 4, 4}, {4, 8, 4}, {8, 4, 4}, {4, 16, 8}, {8, 8, 8}, {16, 4, 8}, {8, 16, 16}, {16, 8, 16}};
  for (const auto& r : slide) {
    const int ck = r[0], co = r[1], wseg = r[2];
    if (ksize == 3 && ((Cin >= 16 && ck == 16) || Cin == ck) && Cin % ck == 0 && Cout == co)
      return Old{fmt("conv_dw_slide_kernel<%d, %d, %d>", ck, co, wseg), false, g, Cin / ck, false};
  }
  if (ksize == 3 && Cin % 16 == 0) {
    if (Cout == 16) return old_run_dw_mfma(16, 1, 16, Cin, g, 0);
    if (Cout == 32) return old_run_dw_mfma(32, 1, 16, Cin, g, 0);
    if (Cout == 64) return old_run_dw_mfma(64, 1, 16, Cin, g, 0);
  }
  if (ksize == 3 && ((Cin == 16 && Cout == 1) || (Cin == 1 && Cout == 16)))
    return Old{Cout == 1 ? "conv_dw_mfma_edge_kernel<0>" : "conv_dw_mfma_edge_kernel<1>", false, g, 1, false};
  // TRY(ck, co, ks) -> run_dw<ck, co, ks>
  static const int tile[20][3] = {{1, 16, 3}, {16, 1, 3}, {4, 4, 3},  {4, 8, 3},   {4, 16, 3},  {8, 4, 3},  {8, 8, 3},
                                  {8, 16, 3}, {8, 32, 3}, {16, 4, 3}, {16, 8, 3},  {16, 16, 3}, {16, 32, 3}, {16, 64, 3},
                                  {16, 4, 1}, {4, 8, 1},  {16, 8, 1}, {8, 16, 1},  {16, 16, 1}, {16, 32, 1}};
  for (const auto& r : tile) {
    const int ck = r[0], co = r[1], ks = r[2];
    if (ksize == ks && ((Cin >= 16 && ck == 16) || Cin == ck) && Cin % ck == 0 && Cout == co)
      return Old{fmt("conv_dw_tile_kernel<%d, %d, %d, 1>", ck, co, ks), false, g, Cin / ck, ks == 1 && ck == 16 && (co == 16 || co == 32)};
  }
  return Old{};
}
static Old old_stride2(int Ca, int Cb, int D, int B, int fine_q4) {
  if (D % 16) return Old{};
  const int g = old_groups_s2(B, D);
  if (Ca % 16 == 0) {
    if (Cb == 16) return old_run_dw_mfma(16, 2, 16, Ca, g, fine_q4);
    if (Cb == 32) return old_run_dw_mfma(32, 2, 16, Ca, g, fine_q4);
    if (Cb == 64) return old_run_dw_mfma(64, 2, 16, Ca, g, fine_q4);
  }
  if (fine_q4) return Old{"generic", true};
  // TRY2(16) TRY2(32) TRY2(64): the same condition as the MFMA rung above, never reached
  return Old{};
}
static bool old_pair_supported(int D, int Cin, int Cout) { return D % 16 == 0 && Cin % 16 == 0 && (Cout == 4 || Cout == 8); }

// the one rename: the 1^3 instantiations of conv_dw_tile_kernel<CIN, COUT, KS, STRIDE> that are kept
static std::string renamed(const std::string& old) {
  static const std::map<std::string, std::string> m = {{"conv_dw_tile_kernel<16, 8, 1, 1>", "conv_dw_tile1_kernel<16, 8>"},
                                                        {"conv_dw_tile_kernel<8, 16, 1, 1>", "conv_dw_tile1_kernel<8, 16>"},
                                                        {"conv_dw_tile_kernel<16, 16, 1, 1>", "conv_dw_tile1_kernel<16, 16>"},
                                                        {"conv_dw_tile_kernel<16, 32, 1, 1>", "conv_dw_tile1_kernel<16, 32>"}};
  const auto it = m.find(old);
  return it == m.end() ? old : it->second;
}

static std::set<std::string> g_kept;                        // names of the enum's kernels
static std::set<int> g_seen;                                // enum values some input got
struct Exception { std::string old_kernel; std::set<int> sizes; };
static std::map<std::string, Exception> g_exceptions;       // by shape
static long g_inputs = 0;

// same kernel, grid, batchable flag and refusal — or an exception: old = a deleted instantiation, new = the generic kernel
static bool compare(const Old& o, const DwChoice& c, const std::string& shape, int D, const char* what) {
  ++g_inputs;
  g_seen.insert((int)c.kernel);
  const std::string old_name = renamed(o.kernel), new_name = dw_kernel_name(c.kernel);
  if (old_name == new_name && o.refused == c.refused) {
    const bool launched = c.kernel != DwKernel::kGeneric;
    CHECK(!launched || (o.groups == c.groups && o.chunks == c.chunks && o.batchable == c.batchable),
          "%s %s D=%d: grid %d x %d batchable %d, was %d x %d batchable %d", what, shape.c_str(), D, c.groups, c.chunks, (int)c.batchable, o.groups,
          o.chunks, (int)o.batchable);
    return true;
  }
  const bool is_exception = !o.refused && !c.refused && c.kernel == DwKernel::kGeneric && !g_kept.count(old_name);
  CHECK(is_exception, "%s %s D=%d: %s%s, was %s%s", what, shape.c_str(), D, new_name.c_str(), c.refused ? " (refused)" : "", o.kernel.c_str(),
        o.refused ? " (refused)" : "");
  if (is_exception) {
    g_exceptions[shape].old_kernel = o.kernel;
    g_exceptions[shape].sizes.insert(D);
  }
  return false;
}

// what a caller sizes (the training plan per layer, the public entry point from kDwPartials) holds what the grid writes
static void check_size(const DwChoice& c, int B, int D_layer, int Cin, int Cout, int ksize, int stride, int transposed, const char* what) {
  if (c.refused || c.kernel == DwKernel::kGeneric) return;
  const size_t wn = (size_t)ksize * ksize * ksize * Cin * Cout, written = (size_t)c.groups * (wn + Cout);
  size_t bias_floats = 0;
  const size_t plan = bwd_weight_partial_floats(B, D_layer, Cin, Cout, ksize, stride, transposed, &bias_floats);
  CHECK(plan >= written, "%s Cin=%d Cout=%d k=%d B=%d D=%d: plan %zu < %zu", what, Cin, Cout, ksize, B, D_layer, plan, written);
  CHECK((size_t)kDwPartials * (wn + 64) >= written, "%s Cin=%d Cout=%d k=%d B=%d D=%d: workspace", what, Cin, Cout, ksize, B, D_layer);
  CHECK(c.groups >= 1 && c.groups <= kDwGroups && c.chunks >= 1, "%s: grid %d x %d", what, c.groups, c.chunks);
}

static const int kBatches[] = {1, 2, 8, 24};

int main(int argc, char** argv) {
  for (int k = 0; k < (int)DwKernel::kCount; ++k) g_kept.insert(dw_kernel_name((DwKernel)k));
  CHECK((int)g_kept.size() == (int)DwKernel::kCount, "kernel names are not distinct");
  static_assert(kDwPartials >= kDwGroups && kDwPartials >= kDwChunks, "workspace slots");

  // 1. the exhaustive grid
  const int chans[] = {1, 2, 4, 8, 16, 32, 48, 64}, sizes[] = {4, 8, 16, 32, 48, 64};
  for (int Cin : chans)
    for (int Cout : chans)
      for (int D : sizes)
        for (int B : kBatches) {
          for (int ksize : {1, 3, 5})
            for (int q = 0; q < 4; ++q) {
              const int x_q4 = q & 1, dz_q4 = q >> 1;
              const DwChoice c = dw_choose(ksize, Cin, Cout, D, B, x_q4, dz_q4);
              compare(old_stride1(ksize, Cin, Cout, D, B, x_q4, dz_q4), c, fmt("stride 1 k=%d %d -> %d", ksize, Cin, Cout), D, "grid");
              check_size(c, B, D, Cin, Cout, ksize, 1, 0, "stride 1");
            }
          for (int fine_q4 = 0; fine_q4 < 2; ++fine_q4) {
            const DwChoice c = dw_choose_s2(Cin, Cout, D, B, fine_q4);
            compare(old_stride2(Cin, Cout, D, B, fine_q4), c, fmt("stride 2 fine %d, coarse %d", Cin, Cout), D, "grid");
            check_size(c, B, 2 * D, Cin, Cout, 3, 2, 0, "stride-2 conv");             // fine = x [2D], coarse = dz [D]
            check_size(c, B, D, Cout, Cin, 3, 2, 1, "transposed conv");                // fine = dz [2D], coarse = x [D]
          }
          const DwChoice c = dw_choose_pair(Cin, Cout, D, B);
          ++g_inputs;
          g_seen.insert((int)c.kernel);
          const bool paired = c.kernel != DwKernel::kGeneric;
          CHECK(paired == old_pair_supported(D, Cin, Cout) && paired == conv_dw_pair_supported(D, Cin, Cout) && !c.refused, "pair %d -> %d D=%d",
                Cin, Cout, D);
          CHECK(!paired || (c.kernel == (Cout == 4 ? DwKernel::kMfma16Pair_4 : DwKernel::kMfma16Pair_8) && c.groups == old_groups(B, D) &&
                            c.chunks == Cin / 16 && !c.batchable), "pair %d -> %d D=%d: kernel or grid", Cin, Cout, D);
          check_size(c, B, D, Cin, Cout, 3, 1, 0, "pair 3^3");
          check_size(c, B, D, Cin, Cout, 1, 1, 0, "pair 1^3");
        }
  std::printf("exceptions (old: a deleted instantiation -> new: the generic kernel):\n");
  for (const auto& e : g_exceptions) {
    std::printf("  EXCEPTION %s: %s -> generic, D =", e.first.c_str(), e.second.old_kernel.c_str());
    for (int D : e.second.sizes) std::printf(" %d", D);
    std::printf("\n");
  }

  // 2. every enum value is somebody's kernel
  for (int k = 0; k < (int)DwKernel::kCount; ++k) CHECK(g_seen.count(k), "%s is never chosen", dw_kernel_name((DwKernel)k));

  // 3. the nets' layers: "<label> <conv|tconv|pair> <cin> <cout> <k> <stride> <D of the layer input> <x_q4> <y_q4>" per line
  long layers = 0;
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "r");
    CHECK(f != nullptr, "cannot read %s", argv[1]);
    char label[128], kind[16];
    int cin, cout, k, stride, D, x_q4, y_q4;
    while (f && std::fscanf(f, "%127s %15s %d %d %d %d %d %d %d", label, kind, &cin, &cout, &k, &stride, &D, &x_q4, &y_q4) == 9) {
      ++layers;
      for (int B : kBatches) {
        bool same = true;
        if (!std::strcmp(kind, "pair")) {
          same = conv_dw_pair_supported(D, cin, cout) == old_pair_supported(D, cin, cout);
        } else if (stride == 1) {
          same = compare(old_stride1(k, cin, cout, D, B, x_q4, y_q4), dw_choose(k, cin, cout, D, B, x_q4, y_q4), label, D, "layer");
        } else if (k == 3 && !std::strcmp(kind, "conv")) {          // bwd_weight_impl: fine = x, coarse = dz on the D / 2 grid
          same = compare(old_stride2(cin, cout, D / 2, B, x_q4), dw_choose_s2(cin, cout, D / 2, B, x_q4), label, D, "layer");
        } else if (k == 3) {                                         // transposed: fine = dz, coarse = x on the D grid
          same = compare(old_stride2(cout, cin, D, B, y_q4), dw_choose_s2(cout, cin, D, B, y_q4), label, D, "layer");
        }                                                            // (other stride-2 filters never come to the tiled kernels)
        CHECK(same, "layer %s (%s %d -> %d k=%d D=%d q4 %d %d) is among the exceptions", label, kind, cin, cout, k, D, x_q4, y_q4);
      }
    }
    if (f) std::fclose(f);
  }
  std::printf("%ld inputs checked, %d kernels, %zu exception shapes, %ld layer records, %ld failures\n", g_inputs, (int)DwKernel::kCount - 1,
              g_exceptions.size(), layers, g_failures);
  return g_failures ? 1 : 0;
}
