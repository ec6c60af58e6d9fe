"""tests/_offgrid_ref.py (brute force over all pairs) against metrics.pc_error_off_grid (k-d tree, scipy) on the scaled-back
pairs: the yardstick of tests/test_gpu_offgrid.py is the rule the host path already follows.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _offgrid_ref as ref                                               # noqa: E402
from pcgcv1_amd import metrics                                           # noqa: E402

CASES = ref.cases()


@pytest.mark.parametrize("name", ["s5_8", "s3_4", "s8_5"])
def test_brute_force_agrees_with_the_host_path(name):
    """Every key within 1e-12 relative: the margin test_gpu_d1d2_exact.py gives float64 sums taken in another order."""
    a, b, na = CASES[name]
    assert metrics._off_grid(b)
    want = metrics.pc_error_off_grid(a, b, na, 1023)
    got = ref.pc_error(a, b, na, 1023)
    assert got["_1"]["n_ties"].max() <= 8 and got["_2"]["n_ties"].max() <= 8          # the host path sees every tie here
    for k, v in want.items():
        print(name, k, got[k], v)
        assert abs(got[k] - v) <= 1e-12 * abs(v), (name, k, got[k], v)
    assert set(k for k in got if not k.startswith("_")) == set(want)


def test_the_cases_hold_what_they_are_there_for():
    """tied targets, an inexact tie and near misses at scale 5/8; a near miss eight times the threshold at 3/4; several
    points per unit cell at 8/5; twelve ties, more than the host path's k = 8"""
    def gaps(name, way):
        a, b, na = CASES[name]
        r = ref.pc_error(a, b, na)
        src, dst = (a, r["_b"]) if way == "1" else (r["_b"], a)
        gap = np.abs(ref.dist2(src, dst) - r["_" + way]["best"][:, None])
        return r, gap, gap < ref.TIE
    r, gap, tie = gaps("s5_8", "1")
    assert (len(CASES["s5_8"][0]), len(r["_b"])) == (1418, 786)
    assert 0.03 < float((r["_1"]["n_ties"] > 1).mean()) < 0.035
    assert 0 < gap[tie & (gap > 0)].max() < 1e-12 and 3e-7 < gap[~tie].min() < 4e-7
    r, gap, tie = gaps("s3_4", "1")
    assert 7.9e-8 < gap[~tie].min() < 8e-8
    b = ref.pc_error(*CASES["s8_5"])["_b"]
    assert np.unique(np.floor(b), axis=0, return_counts=True)[1].max() == 4
    r = ref.pc_error(*CASES["twelve_ties"])
    assert r["_1"]["n_ties"].tolist() == [12] and r["_1"]["best"].tolist() == [4.5]
