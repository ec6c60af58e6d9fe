// Stand-alone audit of the weight-gradient test cases (tests/_dw_cases.py) against csrc/dw_plan.h: g++ -std=c++17 -O1 -Wall
// -Werror, no GPU.  tests/test_dw_cases_host.py builds it and runs it on one record per case:
//   <conv|pair> ksize Cin Cout stride transposed D-of-the-layer-input B expected-generic
// and gets back, per case, the kernel dw_plan.h chooses, its grid, and how many tiles that grid walks:
//   case <index> | <kernel name> | groups | chunks | tiles | voxels
// The tile geometry is restated here from the kernels' headers in train_dw.hip (TD, TH, TW of each template), not taken from
// the launcher: conv_dw_tile_groups is what the launch uses, the tile counts below are what the kernels loop over.
#include <cstdio>
#include <cstring>

#include "../pcgcv1_amd/csrc/dw_plan.h"

using namespace pcgc;

// tiles one workgroup column of the kernel walks with `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)`
static long tiles_of(DwKernel k, int B, int D /* the grid the tiles lie on: coarse for stride 2 */) {
  switch (k) {
    case DwKernel::kGeneric:
    case DwKernel::kCount:
      return 0;
    case DwKernel::kOne_16x4:
    case DwKernel::kOne_4x8:                  // conv_dw_1x1_kernel: thread t of workgroup g takes voxels 256 g + t + n * 256 * groups:
      return (long)B * D * D * D / 256;       // a "tile" is 256 consecutive voxels (D % 16 == 0, so they divide)
    case DwKernel::kMfma4_4:
    case DwKernel::kMfma4_8:                  // conv_dw_mfma_4xn_kernel: TD = 4, TH = 4, TW = 64 = D, ntiles = B * td * th
      return (long)B * (D / 4) * (D / 4);
    case DwKernel::kMfmaS2_16x16:
    case DwKernel::kMfmaS2_16x32:
    case DwKernel::kMfmaS2_16x64:             // conv_dw_mfma_kernel<COUT, 2>: TD = TH = 2, TW = 16 on the coarse grid
      return (long)B * (D / 2) * (D / 2) * (D / 16);
    default:                                  // every other kernel: TD = 4, TH = 4, TW = 16
      return (long)B * (D / 4) * (D / 4) * (D / 16);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: dw_cases_check <cases.txt>\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  char kind[16];
  int ksize, cin, cout, stride, transposed, D, B, generic, index = 0, failures = 0;
  while (std::fscanf(f, "%15s %d %d %d %d %d %d %d %d", kind, &ksize, &cin, &cout, &stride, &transposed, &D, &B, &generic) == 9) {
    DwChoice c;
    int grid_D = D;                           // the grid the kernel's tiles lie on
    long voxels = 0;                          // voxels of the iteration space (what a weight's sum runs over)
    if (!std::strcmp(kind, "pair")) {
      c = dw_choose_pair(cin, cout, D, B);
    } else if (stride == 1 && !transposed) {
      c = dw_choose(ksize, cin, cout, D, B, 0, 0);
    } else if (ksize == 3 && !transposed) {   // bwd_weight_impl (train.hip): fine = x [D], coarse = dz [D / 2]
      grid_D = D / 2;
      c = dw_choose_s2(cin, cout, grid_D, B, 0);
    } else if (ksize == 3) {                  // transposed: fine = dz [2 D] with Cout channels, coarse = x [D] with Cin
      c = dw_choose_s2(cout, cin, D, B, 0);
    } else {                                  // other stride-2 filters never come to the tiled kernels
      grid_D = transposed ? D : D / 2;
    }
    voxels = (long)B * grid_D * grid_D * grid_D;
    if (c.refused) { std::printf("FAIL case %d: refused\n", index); ++failures; }
    long tiles = tiles_of(c.kernel, B, grid_D);
    int groups = c.groups, chunks = c.chunks;
    if (c.kernel == DwKernel::kGeneric) {     // conv_dw_partial_kernel: kDwChunks chunks of ceil(voxels / kDwChunks) voxels each
      groups = kDwChunks;
      chunks = 1;
      tiles = voxels;
    }
    if ((c.kernel == DwKernel::kGeneric) != (generic != 0)) {
      std::printf("FAIL case %d: %s, expected %s\n", index, dw_kernel_name(c.kernel), generic ? "the generic kernel" : "a tiled kernel");
      ++failures;
    }
    std::printf("case %d | %s | %d | %d | %ld | %ld\n", index, dw_kernel_name(c.kernel), groups, chunks, tiles, voxels);
    ++index;
  }
  std::fclose(f);
  std::printf("kernels:");
  for (int k = 1; k < (int)DwKernel::kCount; ++k) std::printf(" | %s", dw_kernel_name((DwKernel)k));
  std::printf("\n%d cases, %d tiled kernels, %d failures\n", index, (int)DwKernel::kCount - 1, failures);
  return failures ? 1 : 0;
}
