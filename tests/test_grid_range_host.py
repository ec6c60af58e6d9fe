"""The Python wrappers of the voxel-grid kernels name the grid's limit before anything touches the device: coordinates
outside [0, 4096) are a ValueError of metrics.d1_metrics, d2_metrics, color_metrics and recolor.recolor, as they are of
metrics.estimate_normals (the library itself only says "bad arguments").  No GPU: the check comes before require_gpu()."""
import numpy as np
import pytest

from pcgcv1_amd import metrics
from pcgcv1_amd import recolor as rc

INSIDE = np.array([[0, 0, 0], [4095, 7, 9]], np.int32)
BAD = {"4096": np.array([[0, 0, 0], [3, 4096, 9]], np.int32), "-1": np.array([[0, -1, 0], [3, 4, 9]], np.int32)}
COL = np.zeros((2, 3), np.uint8)
NRM = np.ones((2, 3), np.float32)


@pytest.mark.parametrize("which", sorted(BAD))
@pytest.mark.parametrize("side", ["a", "b"])
def test_wrappers_name_the_limit(which, side):
    a, b = (BAD[which], INSIDE) if side == "a" else (INSIDE, BAD[which])
    calls = {
        "d1_metrics": lambda: metrics.d1_metrics(a, b, 4095),
        "d2_metrics": lambda: metrics.d2_metrics(a, NRM, b, 4095),
        "color_metrics": lambda: metrics.color_metrics(a, COL, b, COL),
        "pc_error": lambda: metrics.pc_error(a, b, NRM, 4095, colors_a=COL, colors_b=COL),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=r"within \[0, 4096\)") as e:
            call()
        assert which in str(e.value), (name, str(e.value))


def test_recolor_names_the_limit():
    for which, bad in BAD.items():
        with pytest.raises(ValueError, match=r"recolor: coordinates must lie within \[0, 4096\)") as e:
            rc.recolor(bad, COL, INSIDE)                                  # a source point outside
        assert which in str(e.value)
    with pytest.raises(ValueError, match=r"within \[0, 4096\)"):
        rc.recolor(INSIDE, COL, BAD["4096"])                             # a target beyond it: the default resolution is 4097
    with pytest.raises(ValueError, match=r"within \[0, 4096\)"):
        rc.recolor(INSIDE, COL, INSIDE, resolution=4097)
    with pytest.raises(ValueError, match=r"within \[0, resolution = 100\)"):
        rc.recolor(INSIDE, COL, INSIDE, resolution=100)                  # inside the grid's limit, outside the caller's


def test_the_limit_is_the_librarys():
    assert metrics.GRID_MAX_RES == 4096
    metrics.check_grid_range("x", INSIDE, INSIDE)
