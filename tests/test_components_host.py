"""The host side of the component filters (pcgcv1_amd/clean.py: component:MIN[:G], largest[:G]): the spec strings, the rule in
numpy (tests/_components_ref.py) against scipy.ndimage.label and cases worked out by hand, and what the three command lines
accept and refuse.  No GPU."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _components_ref as ref                                            # noqa: E402
from pcgcv1_amd import clean, ingest                                     # noqa: E402
from pcgcv1_amd import test as cli                                       # noqa: E402


def test_parse_spec_accepts():
    s = clean.parse_spec("component:28")
    assert (s.kind, s.min_count, s.gap, s.text) == ("component", 28, 1, "component:28")
    s = clean.parse_spec("component:1:8")
    assert (s.kind, s.min_count, s.gap) == ("component", 1, 8)
    s = clean.parse_spec("largest")
    assert (s.kind, s.gap, s.text) == ("largest", 1, "largest")
    s = clean.parse_spec("largest:2")
    assert (s.kind, s.gap) == ("largest", 2) and repr(s) == "Spec('largest:2')"
    assert clean.parse_spec("component:%d" % (2 ** 31 - 1)).min_count == 2 ** 31 - 1
    assert clean.MAX_GAP == 8 and clean.parse_spec(s) is s
    # the gap is part of what makes two specs equal; the old kinds have one too, and compare as before
    assert clean.parse_spec("largest") != clean.parse_spec("largest:2") and clean.parse_spec("largest") == clean.parse_spec("largest:1")
    assert clean.parse_spec("component:5") != clean.parse_spec("component:5:2")
    assert clean.parse_spec("stat:20:2.0").gap == clean.parse_spec("radius:2:5").gap == 1
    assert clean.parse_specs(["stat:20:2.0", "largest:2"])[1].kind == "largest"
    assert [ref.parse_spec(t) for t in ("component:28", "component:6:2", "largest", "largest:2", "radius:2:5")] == [
        ("component", 28, 1), ("component", 6, 2), ("largest", 1), ("largest", 2), ("radius", 2, 5)]


@pytest.mark.parametrize("text, field", [
    ("component", "fields"), ("component:0", "MIN = 0"), ("component:5:0", "G = 0"), ("component:5:9", "G = 9"),
    ("component:x", "MIN = 'x'"), ("component:5:1:1", "fields"), ("component:%d" % 2 ** 31, "MIN = %d" % 2 ** 31),
    ("largest:0", "G = 0"), ("largest:9", "G = 9"), ("largest:1:1", "fields"), ("largest:two", "G = 'two'"),
])
def test_parse_spec_refuses(text, field):
    with pytest.raises(ValueError) as e:
        clean.parse_spec(text)
    assert field in str(e.value) and "--clean " + text in str(e.value)


def test_an_unknown_kind_names_all_four():
    with pytest.raises(ValueError) as e:
        clean.parse_spec("components:5")
    for word in ("neither", "'radius'", "'stat'", "'component'", "'largest'", "--clean components:5"):
        assert word in str(e.value)


def test_reference_by_hand():
    # bits = 3.  A pair one diagonal step apart, a voxel two cells from it along x, and one far away
    p = np.array([[1, 1, 1], [2, 2, 2], [4, 2, 2], [7, 7, 0]])
    label, size, n = ref.components(p, 3, 1)
    assert label.dtype == np.int64 and size.dtype == np.int32
    assert n == 3 and label.tolist() == [73, 73, 4 * 64 + 2 * 8 + 2, 7 * 64 + 7 * 8] and size.tolist() == [2, 2, 1, 1]
    label, size, n = ref.components(p, 3, 2)
    assert n == 2 and label.tolist() == [73, 73, 73, 504] and size.tolist() == [3, 3, 3, 1]
    label, size, n = ref.components(p, 3, 5)                             # (4,2,2) -> (7,7,0): five cells along y
    assert n == 1 and label.tolist() == [73] * 4 and size.tolist() == [4] * 4
    # nothing wraps: (0,0,7) and (0,1,0) have adjacent keys and lie seven cells apart
    assert ref.components(np.array([[0, 0, 7], [0, 1, 0]]), 3, 1)[2] == 2
    assert ref.components(np.array([[0, 7, 3], [1, 0, 3]]), 3, 1)[2] == 2
    assert ref.components(np.array([[7, 7, 7], [0, 0, 0]]), 3, 1)[2] == 2
    assert ref.keys([[1, 2, 3]], 4).tolist() == [(1 * 16 + 2) * 16 + 3]


def test_reference_masks():
    block = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = np.r_[block + 4, block, [[0, 0, 3]], [[15, 15, 15]]]            # bits = 4: two 2^3 blocks, a voxel two cells from one, a lone one
    assert ref.keep_mask(p, 4, "component:8").tolist() == [True] * 16 + [False, False]
    assert ref.keep_mask(p, 4, "component:9").sum() == 0 and ref.keep_mask(p, 4, "component:9:2").tolist() == [False] * 8 + [True] * 9 + [False]
    assert ref.keep_mask(p, 4, "largest").tolist() == [False] * 8 + [True] * 8 + [False, False]     # a tie: the smaller label
    assert ref.keep_mask(p, 4, "largest:2").tolist() == [False] * 8 + [True] * 9 + [False]
    assert ref.keep_mask(p, 4, "largest:3").sum() == 17                 # (1,1,1) and (4,4,4) are three cells apart
    assert ref.keep_mask_all(p, 4, ["component:2:2", "largest"]).tolist() == [False] * 8 + [True] * 8 + [False, False]
    assert ref.keep_mask_all(p, 4, ["radius:1:1", "largest:2"]).tolist() == [False] * 8 + [True] * 8 + [False, False]


def test_reference_against_scipy_on_the_surface():
    p = ref.surface()
    assert len(p) == 3159
    label, size, n = ref.components(p, 6, 1)
    grid = np.zeros((64, 64, 64), bool)
    grid[p[:, 0], p[:, 1], p[:, 2]] = True
    lab, count = ndimage.label(grid, structure=np.ones((3, 3, 3)))
    assert n == count == 768
    mine = lab[p[:, 0], p[:, 1], p[:, 2]]
    # the same partition: one of scipy's labels per label of ours and the other way round
    pairs = np.unique(np.stack([mine, label], 1), axis=0)
    assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
    np.testing.assert_array_equal(size, np.bincount(mine)[mine])
    assert size.max() == 125                                            # at G = 1 the largest component is the block
    for gap, want_n, want_max in ((2, 28, 3002), (3, 22, 3012), (8, 6, 3028)):
        _, size, n = ref.components(p, 6, gap)
        assert (n, size.max()) == (want_n, want_max)


@pytest.mark.parametrize("bits, n", [(3, 143), (4, 1087), (5, 8447)])
def test_snake_generator(bits, n):
    s = ref.snake(bits)
    assert len(s) == n and len(np.unique(s, axis=0)) == n and s.min() == 0 and s.max() == (1 << bits) - 1
    assert (np.abs(np.diff(s, axis=0)).sum(1) == 1).all()               # consecutive cells are one step apart
    assert ref.keys(s, bits).min() == 0


def test_components_line():
    label = np.array([5, 5, 9, 5, 40, 9, 77, -1], np.int64)
    size = np.array([3, 3, 2, 3, 1, 2, 1, 0], np.int32)
    assert clean.components_line(clean.parse_spec("largest:2"), label, size) == "components: largest:2 saw 4 components, the largest of 3 2 1 voxels"
    assert clean.components_line(clean.parse_spec("component:2"), label[:2], size[:2]) == "components: component:2 saw 1 components, the largest of 3 voxels"


# ---------------------------------------------------------------------------- the three command lines
IO = ["--input", "a.ply", "--output", "b.ply"]
BAD = ["component", "component:0", "component:5:0", "component:5:9", "component:x", "component:5:1:1", "largest:0", "largest:9", "largest:1:1"]


def test_the_command_lines_accept(capsys):
    a = clean.parse_args(IO + ["--clean", "stat:20:2.0", "--clean", "largest:2"])
    assert [s.text for s in a.clean] == ["stat:20:2.0", "largest:2"] and a.clean[1].gap == 2
    a = ingest.parse_args(IO + ["--bits", "10", "--clean", "component:28", "--clean", "largest"])
    assert [(s.kind, s.min_count, s.gap) for s in a.clean] == [("component", 28, 1), ("largest", 0, 1)]
    a = cli.parse_args(["compress", "x.ply", "--voxelize", "7", "--clean", "component:6:2"])
    assert a.clean == [clean.parse_spec("component:6:2")]
    a = cli.parse_args(["compress", "x.ply", "--clean", "largest:8"])
    assert a.clean[0].gap == 8
    for parser in (clean.parse_args, ingest.parse_args):
        with pytest.raises(SystemExit) as e:
            parser(["--help"])
        assert e.value.code == 0
        said = " ".join(capsys.readouterr().out.split())
        assert "component:MIN[:G]" in said and "largest[:G]" in said


@pytest.mark.parametrize("text", BAD)
def test_the_command_lines_refuse(text, capsys):
    for parser, argv in ((clean.parse_args, IO), (ingest.parse_args, IO + ["--bits", "10"]), (cli.parse_args, ["compress", "x.ply"])):
        with pytest.raises(SystemExit) as e:
            parser(argv + ["--clean", text])
        assert e.value.code == 2 and "--clean " + text in capsys.readouterr().err
