"""The weight-gradient launches tests/test_gpu_train_dw.py runs and tests/test_dw_cases_host.py audits on the CPU.

A case is (ksize, Cin, Cout, stride, transposed, D of the layer input, B) for pcgc_conv3d_bwd_weight, or
("pair", Cin, Cout, D, B) for conv1_1 + conv2_1 of a VRN block through pcgc_train_conv_bwd_weight_pair.

The tiled kernels of train_dw.hip are persistent: at most kDwGroups = 512 workgroups, each walking tiles blockIdx.x,
blockIdx.x + gridDim.x, ...  The sizes below are the smallest at which every kernel of csrc/dw_plan.h gets MORE tiles than
workgroups and a tile count that is NO multiple of the workgroup count, so that some workgroups run one more iteration than
others (and the prefetch guards differ across the grid in the last round).  They are not the workload's sizes.  D = 48 where
it works: three tiles along w, so the tile-index decode meets a non-power-of-two.  test_dw_cases_host.py asserts the coverage
(tests/dw_cases_check.cpp restates the tile geometry); the comments give tiles / workgroups as that program prints them.
"""

TILED_CASES = [
    # conv_dw_mfma_4xn_kernel<4>, <8>: D = 64 only, whole-row tiles (4 x 4 x 64), 256 B tiles for 512 workgroups
    (3, 4, 4, 1, 0, 64, 3), (3, 4, 8, 1, 0, 64, 3),             # 768 / 512
    (3, 4, 4, 1, 0, 64, 1), (3, 4, 8, 1, 0, 64, 1),             # 256 / 512: half of the workgroups write a partial of zeros
    # conv_dw_mfma_16xn_kernel<4, false>, <8, false>: two channel chunks
    (3, 32, 4, 1, 0, 48, 2), (3, 32, 8, 1, 0, 48, 2),           # 864 / 512
    # conv_dw_mfma_kernel<16, 1, 8>, conv_dw_slide_kernel<4, 4, 4>, <4, 8, 4>, <8, 8, 8>
    (3, 8, 16, 1, 0, 48, 2), (3, 4, 4, 1, 0, 48, 2), (3, 4, 8, 1, 0, 48, 2), (3, 8, 8, 1, 0, 48, 2),
    # conv_dw_mfma_kernel<16, 1, 16> (two chunks), <32, 1, 16> (two chunks), <64, 1, 16>
    (3, 32, 16, 1, 0, 48, 2),
    (3, 32, 32, 1, 0, 32, 5), (3, 16, 64, 1, 0, 32, 5),         # 640 / 512
    # conv_dw_mfma_edge_kernel<0>, <1>
    (3, 16, 1, 1, 0, 48, 2), (3, 1, 16, 1, 0, 48, 2),
    # conv_dw_tile1_kernel<16, 8> (two chunks), <8, 16>, <16, 16> (two chunks), <16, 32>
    (1, 32, 8, 1, 0, 48, 2), (1, 8, 16, 1, 0, 32, 5), (1, 32, 16, 1, 0, 48, 2), (1, 16, 32, 1, 0, 32, 5),
    # conv_dw_1x1_kernel<16, 4>, <4, 8>: 552 960 voxels = 4.2 strides of 512 x 256 threads: a second round of U = 4 strides
    # that ends inside a stride
    (1, 16, 4, 1, 0, 48, 5), (1, 4, 8, 1, 0, 48, 5),
    # conv_dw_mfma_kernel<16 / 64 / 32, 2, 16> as the stride-2 conv (x on the fine grid): 2 x 2 x 16 tiles of the coarse grid
    (3, 16, 16, 2, 0, 96, 1), (3, 32, 64, 2, 0, 96, 1),         # 1728 / 512
    (3, 16, 32, 2, 0, 32, 17),                                  # 1088 / 512
    # the same three as the transposed conv (dz on the fine grid; the kernel's Cout is the layer's Cin)
    (3, 16, 16, 2, 1, 48, 1), (3, 32, 16, 2, 1, 48, 1),         # 1728 / 512
    (3, 64, 32, 2, 1, 16, 17),                                  # 1088 / 512
]

PAIR_CASES = [
    ("pair", 32, 4, 48, 2),                                     # conv_dw_mfma_16xn_kernel<4, true>: 864 / 512
    ("pair", 32, 8, 32, 5),                                     # conv_dw_mfma_16xn_kernel<8, true>: 640 / 512
]

# conv_dw_partial_kernel (train.hip), 128 voxel chunks of ceil(voxels / 128) each: shapes dw_plan.h has no row for
GENERIC_CASES = [
    (3, 8, 32, 1, 0, 24, 3),     # 41 472 voxels: 128 chunks of 324 = five 64-voxel passes and a ragged sixth of 4
    (3, 8, 4, 1, 0, 20, 3),      # 24 000 voxels: chunks of 188, the last one 124: no multiple of the 128 chunks
    (5, 32, 32, 2, 0, 8, 3),     # 192 output voxels: chunks of 2, the last 32 of the 128 chunks empty
]

CASES = TILED_CASES + PAIR_CASES + GENERIC_CASES


def case_id(case):
    if case[0] == "pair":
        return "pair-%dto%d-D%d-B%d" % case[1:]
    k, cin, cout, stride, tr, D, B = case
    return "k%d-%dto%d-%s-D%d-B%d" % (k, cin, cout, "tconv" if tr else "s%d" % stride, D, B)


def case_line(case):
    """The record tests/dw_cases_check.cpp reads: kind ksize Cin Cout stride transposed D B generic."""
    if case[0] == "pair":
        return "pair 3 %d %d 1 0 %d %d 0" % case[1:]
    return "conv %d %d %d %d %d %d %d %d" % (tuple(case) + (int(case in GENERIC_CASES),))
