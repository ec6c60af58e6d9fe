"""The host side of --clean (pcgcv1_amd/clean.py, its flags in ingest.py and test.py): the rule in numpy (tests/_clean_ref.py)
against cases worked out by hand, the spec strings, the threshold expression and the refusals of the three command lines.
No GPU.

Closed forms used below.  isqrt16(m * m) = m << 16 exactly; isqrt16(2) = floor(65536 * sqrt 2) = 92681, isqrt16(3) =
floor(65536 * sqrt 3) = 113511.  Around the centre of a full 3^3 block lie 6 face neighbours at d2 = 1, 12 edge neighbours
at d2 = 2 and 8 corner neighbours at d2 = 3: 6 inside R = 1 (d2 <= 1, not 26: the ball is Euclidean), all 26 inside R = 2.
Around a corner of the block: 3 at d2 = 1, 3 at d2 = 2, 1 at d2 = 3, 3 at d2 = 4 (the far ends of its three edges): 10 inside
R = 2."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _clean_ref as ref                                                 # noqa: E402
from pcgcv1_amd import clean, ingest                                     # noqa: E402
from pcgcv1_amd import test as cli                                       # noqa: E402

ONE = 1 << 16
BLOCK = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3) + 5       # centre (6, 6, 6) is row 13


def test_isqrt16_values():
    assert [ref.isqrt16(d) for d in (0, 1, 2, 3, 4, 9, 1024)] == [0, ONE, 92681, 113511, 2 * ONE, 3 * ONE, 32 * ONE]
    for d in (2, 3, 5, 1023):
        r = ref.isqrt16(d)
        assert r * r <= d << 32 < (r + 1) * (r + 1) and r == math.isqrt(d << 32)


def test_three_collinear_voxels():
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]])
    S, cnt = ref.neighbor_statistics(pts, 2, 2)
    assert cnt.tolist() == [1, 2, 1] and cnt.dtype == np.int32 and S.dtype == np.int64
    # the end voxels find one neighbour inside R = 2 (at d2 = 1 and at d2 = 4); the second is charged R + 1 = 3
    assert S.tolist() == [ONE + 3 * ONE, ONE + 2 * ONE, 2 * ONE + 3 * ONE]
    S, cnt = ref.neighbor_statistics(pts, 2, 3)                         # R = 3: the d2 = 9 pair is inside too
    assert cnt.tolist() == [2, 2, 2] and S.tolist() == [ONE + 3 * ONE, ONE + 2 * ONE, 2 * ONE + 3 * ONE]
    S, cnt = ref.neighbor_statistics(pts, 1, 1)
    assert cnt.tolist() == [1, 1, 0] and S.tolist() == [ONE, ONE, 2 * ONE]


def test_full_block():
    S, cnt = ref.neighbor_statistics(BLOCK, 8, 1)
    assert cnt[13] == 6 and S[13] == 6 * ONE + 2 * (2 * ONE)            # k > cnt: two of the eight are missing, charged R + 1 = 2
    assert cnt[0] == 3 and S[0] == 3 * ONE + 5 * (2 * ONE)
    S, cnt = ref.neighbor_statistics(BLOCK, 26, 2)
    assert cnt[13] == 26 and S[13] == 6 * ONE + 12 * 92681 + 8 * 113511
    assert cnt[0] == 10 and S[0] == 3 * ONE + 3 * 92681 + 113511 + 3 * (2 * ONE) + 16 * (3 * ONE)
    assert ref.neighbor_statistics(BLOCK, 0, 32)[1].tolist() == [26] * 27


def test_a_tie_at_the_kth_distance():
    # six neighbours at the same distance and k = 3: whichever three are taken, the sum is the same
    assert ref.neighbor_statistics(BLOCK, 3, 1)[0][13] == 3 * ONE
    assert ref.neighbor_statistics(BLOCK, 7, 2)[0][13] == 6 * ONE + 92681      # one of the twelve at d2 = 2
    assert ref.neighbor_statistics(BLOCK, 19, 2)[0][13] == 6 * ONE + 12 * 92681 + 113511


def test_a_lone_voxel():
    for k, R in ((1, 1), (8, 8), (64, 32)):
        S, cnt = ref.neighbor_statistics(np.array([[4, 5, 6]]), k, R)
        assert S.tolist() == [k * ((R + 1) << 16)] and cnt.tolist() == [0]
    S, cnt = ref.neighbor_statistics(np.array([[0, 0, 0], [40, 0, 0]]), 5, 32)     # out of each other's reach
    assert S.tolist() == [5 * 33 * ONE] * 2 and cnt.tolist() == [0, 0]


def test_reference_filters():
    pts = np.r_[BLOCK, [[20, 20, 20]], [[20, 20, 21]]]
    assert ref.keep_mask(pts, "radius:1:3").tolist() == [True] * 27 + [False, False]
    assert ref.keep_mask(pts, "radius:1:4").sum() == 19                 # the eight corners of the block have three
    # S at k = 2, R = 2: 2 * ONE for the block's voxels, ONE + 3 * ONE for the pair
    S = ref.neighbor_statistics(pts, 2, 2)[0]
    assert S.tolist() == [2 * ONE] * 27 + [4 * ONE] * 2
    assert ref.keep_mask(pts, "stat:2:1.0:2").tolist() == [True] * 27 + [False, False]
    assert ref.keep_mask(pts, "stat:2:4.0:2").all()
    # in order, each on what the one before kept: without the pair, the corners are the outliers of the next filter
    assert ref.keep_mask_all(pts, ["radius:1:3", "radius:1:4"]).sum() == 19
    assert ref.keep_mask_all(pts, ["radius:1:4", "radius:1:4"]).sum() == 7       # then the edges have only their two face centres


def test_threshold_expression():
    S = np.array([1, 1, 1, 5], np.int64)
    assert clean.threshold(S, 0.0) == 2.0 and clean.threshold(S, 1.0) == 2.0 + np.sqrt(3.0)      # population std: ddof = 0
    big = np.random.default_rng(0).integers(0, 64 * 33 * ONE, 100001)
    assert clean.threshold(big, 2.5) == np.mean(big) + 2.5 * np.std(big)
    assert (big <= clean.threshold(big, 0.0)).sum() not in (0, len(big))


def test_parse_spec_accepts():
    s = clean.parse_spec("stat:20:2.0")
    assert (s.kind, s.k, s.ratio, s.radius, s.text) == ("stat", 20, 2.0, 8, "stat:20:2.0")
    s = clean.parse_spec("stat:64:0:32")
    assert (s.kind, s.k, s.ratio, s.radius) == ("stat", 64, 0.0, 32)
    s = clean.parse_spec("stat:1:1e-3:1")
    assert (s.k, s.ratio, s.radius) == (1, 0.001, 1)
    s = clean.parse_spec("radius:2:5")
    assert (s.kind, s.radius, s.min_count, s.text) == ("radius", 2, 5, "radius:2:5")
    assert clean.parse_spec("radius:1:26").min_count == 26 and clean.parse_spec(s) is s
    assert clean.parse_specs("radius:2:5") == [s] and clean.parse_specs(["radius:2:5", "stat:8:2"])[1].k == 8
    assert [ref.parse_spec(t) for t in ("stat:20:2.0", "radius:2:5")] == [("stat", 20, 2.0, 8), ("radius", 2, 5)]


@pytest.mark.parametrize("text, field", [
    ("", "neither"), ("median:3", "neither"), ("stat", "fields"), ("stat:8", "fields"), ("stat:8:2:8:1", "fields"),
    ("radius:2", "fields"), ("radius:2:5:1", "fields"),
    ("stat:0:2.0", "K = 0"), ("stat:65:2.0", "K = 65"), ("stat:x:2.0", "K = 'x'"), ("stat:8.5:2.0", "K = '8.5'"),
    ("stat:8:-1", "RATIO"), ("stat:8:nan", "RATIO"), ("stat:8:inf", "RATIO"), ("stat:8:two", "RATIO"),
    ("stat:8:2.0:0", "R = 0"), ("stat:8:2.0:33", "R = 33"), ("radius:0:1", "R = 0"), ("radius:33:1", "R = 33"),
    ("radius:1:0", "MIN = 0"), ("radius:1:27", "MIN = 27"), ("radius:1:-2", "MIN = -2"), ("radius:1:many", "MIN = 'many'"),
])
def test_parse_spec_refuses(text, field):
    with pytest.raises(ValueError) as e:
        clean.parse_spec(text)
    assert field in str(e.value) and "--clean " + text in str(e.value)


def test_bits_for():
    assert clean.bits_for(np.array([[0, 0, 0]])) == 1 and clean.bits_for(np.array([[1, 0, 0]])) == 1
    assert clean.bits_for(np.array([[2, 0, 0]])) == 2 and clean.bits_for(np.array([[0, 127, 3]])) == 7
    assert clean.bits_for(np.array([[0, 128, 3]])) == 8 and clean.bits_for(np.array([[4095, 0, 0]])) == 12
    for bad in (np.array([[4096, 0, 0]]), np.array([[0, -1, 0]]), np.zeros((0, 3), np.int32)):
        with pytest.raises(ValueError):
            clean.bits_for(bad)


def test_summary_line():
    line = clean.summary_line(["stat:20:2.0", "radius:2:3"], 183004, 412, 391, 207, 455)
    assert line == "clean: stat:20:2.0 radius:2:3 removed 412 of 183004 voxels (455 input points); 64^3 cubes 391 -> 207"
    assert clean.summary_line("radius:2:3", 10, 1, 2, 1) == "clean: radius:2:3 removed 1 of 10 voxels; 64^3 cubes 2 -> 1"
    assert clean.n_cubes(np.array([[0, 0, 0], [63, 63, 63], [64, 0, 0], [127, 1, 1]])) == 2


# ---------------------------------------------------------------------------- the three command lines
IO = ["--input", "a.ply", "--output", "b.ply"]


@pytest.mark.parametrize("argv", [
    IO,                                                                  # nothing to do
    IO + ["--clean", "stat:0:2.0"],
    IO + ["--clean", "radius:2:5", "--clean", "radius:2"],               # the second one is wrong
    IO + ["--clean"],
    ["--input", "a.ply", "--clean", "radius:2:5"],
])
def test_clean_cli_refuses_bad_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        clean.parse_args(argv)
    assert e.value.code == 2
    if "--clean" in argv and len(argv) > 5 and argv[-1] != "--clean":
        assert "--clean " + argv[-1] in capsys.readouterr().err


def test_clean_cli_accepts():
    a = clean.parse_args(IO + ["--clean", "stat:20:2.0", "--clean", "radius:2:5"])
    assert [s.text for s in a.clean] == ["stat:20:2.0", "radius:2:5"] and a.clean[0].radius == 8


@pytest.mark.parametrize("argv", [
    IO + ["--bits", "10", "--clean", "stat:8"],
    IO + ["--bits", "10", "--clean", "radius:40:1"],
    IO + ["--voxel_size", "0.5", "--clean", "stat:8:-2"],
    IO + ["--clean", "stat:8:2.0"],                                      # still needs --bits or --voxel_size
])
def test_ingest_cli_refuses_bad_arguments(argv):
    with pytest.raises(SystemExit) as e:
        ingest.parse_args(argv)
    assert e.value.code == 2


def test_ingest_cli_accepts():
    assert ingest.parse_args(IO + ["--bits", "10"]).clean is None
    a = ingest.parse_args(IO + ["--voxel_size", "0.5", "--clean", "stat:8:2.0", "--clean", "radius:1:1"])
    assert [s.text for s in a.clean] == ["stat:8:2.0", "radius:1:1"]


@pytest.mark.parametrize("argv, word", [
    (["compress", "x.ply", "--clean", "stat:8"], "fields"),
    (["compress", "x.ply", "--voxelize", "7", "--clean", "radius:2:0"], "MIN"),
    (["decompress", "compressed/x", "--clean", "stat:8:2.0"], "compress"),
    (["compress", "x.ply", "--clean", "stat:8:2.0", "--scale", "0.5"], "scale"),
    (["compress", "x.ply", "--clean", "stat:8:2.0", "--gpu", "2"], "one GPU"),
])
def test_codec_cli_refuses_bad_arguments(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_codec_cli_mentions_the_flag_only_when_it_is_given(capsys):
    with pytest.raises(SystemExit):
        cli.main(["compress", "scan.ply", "--gpu", "0"])
    line = capsys.readouterr().out.splitlines()[0]
    assert line.startswith("Namespace(command='compress'") and "clean" not in line
    with pytest.raises(SystemExit):
        cli.main(["compress", "scan.ply", "--gpu", "0", "--clean", "stat:20:2.0", "--clean", "radius:2:3"])
    assert "clean=[Spec('stat:20:2.0'), Spec('radius:2:3')]" in capsys.readouterr().out.splitlines()[0]


def test_a_frame_and_clean_do_not_go_together():
    with pytest.raises(ValueError, match="refits"):
        ingest.voxelize_scan(np.zeros((2, 3)), frame=ingest.Frame((0, 0, 0), 1.0, 3), clean="stat:8:2.0")
