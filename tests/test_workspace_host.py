"""Workspaces on the CPU (pcgcv1_amd/csrc/workspace.h): tests/workspace_check.cpp checks the carver every layout function is
written with, and every pcgc_*_workspace_bytes built on it still returns the size it returned when the size was a hand-written
sum (recorded from a build of commit 7a72c4e, the last one with the sums).  libpcgc_hip.so loads without a device."""
import itertools
import os
import subprocess

from pcgcv1_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


def test_carver_regions(tmp_path):
    """Null base: null pointers and the same size; regions 256-aligned, back to back, disjoint, inside bytes(); a zero count
    takes nothing; the unrounded take leaves the size unrounded; a carver handed on goes on where it stood."""
    exe = str(tmp_path / "workspace_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "workspace_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " layouts checked, 0 failures" in run.stdout


# The smallest arguments at which the arithmetic can go wrong.  A scan block holds 131 072 cells: bits 5 -> 6 and res 50 -> 51 cross
# from one block to two (the surface lattices, res + 2 and res + 3, cross there too); bits 12 / res 1024 are the largest grids
# (2^36 / 2^30 cells).  Counts 1, 63, 64, 65 stand on both sides of the 256-byte boundary of a 4-byte region; pairs are unequal.
COUNTS = (1, 63, 64, 65, 2500)
PAIRS = ((1, 1), (63, 64), (64, 65), (65, 63), (2500, 1))
BITS_N = tuple(itertools.product((1, 5, 6), COUNTS)) + ((12, 2500),)
RES_N = tuple(itertools.product((2, 50, 51), COUNTS)) + ((1024, 2500),)
RES_PAIRS = tuple((r,) + p for r in (2, 50, 51) for p in PAIRS) + ((1024, 2500, 1),)

# entry point -> (argument sets, one refused set)
CASES = {
    "pcgc_surface_workspace_bytes": (BITS_N, (13, 1)),
    "pcgc_clean_workspace_bytes": (BITS_N, (0, 1)),
    "pcgc_clean_components_workspace_bytes": (BITS_N, (1, 0)),
    "pcgc_ingest_workspace_bytes": (BITS_N, (13, 1)),
    "pcgc_offgrid_workspace_bytes": (RES_N, (1025, 1)),
    "pcgc_register_workspace_bytes": (RES_N, (2, 0)),               # n_sums = 45
    "pcgc_register_color_workspace_bytes": (RES_N, (0, 1)),         # n_sums = 59
    "pcgc_feature_workspace_bytes": (RES_N, (1025, 1)),
    "pcgc_smooth_workspace_bytes": (RES_N, (2, 0)),
    "pcgc_color_gradient_workspace_bytes": (RES_N, (0, 1)),
    "pcgc_color_mse_workspace_bytes": (RES_N, (4097, 1)),
    "pcgc_recolor_workspace_bytes": (RES_PAIRS, (2, 0, 1)),
    "pcgc_meshdist_workspace_bytes": (RES_PAIRS, (2, 1, 0)),
    "pcgc_mesh_voxelize_workspace_bytes": (((2,), (49,), (50,), (1024,)), (4096,)),       # a grid of (resolution + 1)^3
    "pcgc_normals_workspace_bytes": (tuple(a + (r,) for a in RES_N for r in (1.0, 10.0)), (2, 1, 17.0)),
    "pcgc_pointnums_curves_workspace_bytes": (PAIRS + ((0, 0),), None),      # refuses nothing: its entry point checks the counts
    "pcgc_pointnums_curves_d2_workspace_bytes": (PAIRS + ((0, 0),), None),
    "pcgc_pointnums_normals_workspace_bytes": (tuple((n,) for n in (0,) + COUNTS), None),
    "pcgc_rans_workspace_bytes": (tuple(itertools.product(COUNTS, (1, 32))), (1, 0)),
    "pcgc_raht_workspace_bytes": (tuple((m,) for m in COUNTS + (200, 100000)), (0,)),      # from 193 leaves on the tree top is the larger use
    "pcgc_feature_match_workspace_bytes": (tuple((n,) for n in COUNTS), (0,)),
}

# recorded from commit 7a72c4e, in the order of the argument sets above
PARENT_BYTES = {
    "pcgc_surface_workspace_bytes": (84992, 86272, 86272, 86784, 159488, 84992, 86272, 86272, 86784, 159488, 216064, 217344,
        217344, 217856, 290560, 43016929792),
    "pcgc_clean_workspace_bytes": (16384, 16384, 16384, 16384, 16384, 16384, 16384, 16384, 16384, 16384, 32768, 32768, 32768,
        32768, 32768, 8589934592),
    "pcgc_clean_components_workspace_bytes": (34304, 34560, 34560, 35328, 74240, 34304, 34560, 34560, 35328, 74240, 67072,
        67328, 67328, 68096, 107008, 17184104704),
    "pcgc_ingest_workspace_bytes": (34048, 35840, 35840, 36608, 133888, 34048, 35840, 35840, 36608, 133888, 66816, 68608,
        68608, 69376, 166656, 17184164352),
    "pcgc_offgrid_workspace_bytes": (67328, 68864, 69120, 69888, 167168, 67328, 68864, 69120, 69888, 167168, 100096, 101632,
        101888, 102656, 199936, 268635136),
    "pcgc_register_workspace_bytes": (435968, 437504, 437760, 438528, 535808, 435968, 437504, 437760, 438528, 535808, 468736,
        470272, 470528, 471296, 568576, 269003776),
    "pcgc_register_color_workspace_bytes": (550656, 552192, 552448, 553216, 650496, 550656, 552192, 552448, 553216, 650496,
        583424, 584960, 585216, 585984, 683264, 269118464),
    "pcgc_feature_workspace_bytes": (34048, 34304, 34560, 34816, 64000, 34048, 34304, 34560, 34816, 64000, 66816, 67072, 67328,
        67584, 96768, 268531968),
    "pcgc_smooth_workspace_bytes": (34048, 34304, 34560, 34816, 64000, 34048, 34304, 34560, 34816, 64000, 66816, 67072, 67328,
        67584, 96768, 268531968),
    "pcgc_color_gradient_workspace_bytes": (34048, 34304, 34560, 34816, 64000, 34048, 34304, 34560, 34816, 64000, 66816, 67072,
        67328, 67584, 96768, 268531968),
    "pcgc_color_mse_workspace_bytes": (58112, 58112, 58112, 58368, 68096, 58112, 58112, 58112, 58368, 68096, 90880, 90880,
        90880, 91136, 100864, 268536064),
    "pcgc_recolor_workspace_bytes": (33792, 34560, 34816, 34816, 43776, 33792, 34560, 34816, 34816, 43776, 66560, 67328, 67584,
        67584, 76544, 268511744),
    "pcgc_meshdist_workspace_bytes": (67328, 67584, 68096, 68352, 107264, 67328, 67584, 68096, 68352, 107264, 100096, 100352,
        100864, 101120, 140032, 268575232),
    "pcgc_mesh_voxelize_workspace_bytes": (25088, 25088, 41472, 134701568),
    "pcgc_normals_workspace_bytes": (18176, 34816, 21760, 38400, 21760, 38400, 22784, 39424, 197888, 214528, 18176, 34816,
        21760, 38400, 21760, 38400, 22784, 39424, 197888, 214528, 34560, 51200, 38144, 54784, 38144, 54784, 39168, 55808,
        214272, 230912, 134464512, 134481152),
    "pcgc_pointnums_curves_workspace_bytes": (1792, 2304, 2560, 3840, 81664, 256),
    "pcgc_pointnums_curves_d2_workspace_bytes": (1792, 2304, 2560, 3840, 81664, 256),
    "pcgc_pointnums_normals_workspace_bytes": (256, 256, 256, 256, 512, 10240),
    "pcgc_rans_workspace_bytes": (640, 4608, 24448, 274432, 24832, 278784, 25472, 283392, 970240, 10890240),
    "pcgc_raht_workspace_bytes": (768, 768, 768, 768, 10240, 1024, 400128),
    "pcgc_feature_match_workspace_bytes": (256, 512, 512, 768, 20224),
}


def test_workspace_sizes_are_the_recorded_ones():
    lib = _lib.hip()
    assert sorted(PARENT_BYTES) == sorted(CASES)
    for name, (arg_sets, refused) in CASES.items():
        fn = getattr(lib, name)
        got = tuple(int(fn(*args)) for args in arg_sets)
        assert got == PARENT_BYTES[name], (name, [(a, g, w) for a, g, w in zip(arg_sets, got, PARENT_BYTES[name]) if g != w])
        if refused is not None:
            assert int(fn(*refused)) == 0, (name, refused)
