"""tests/_grid_ref.py (the stencil reference of tests/test_gpu_grid_range.py) against the brute-force references on their small
cases: _dist2 and _plane of tests/test_gpu_d1d2_exact.py, tests/_color_ref.py.  Integers equal; float64 sums within 1e-12
relative, the margin those tests use.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as cref                                                # noqa: E402
import _grid_ref as gref                                                 # noqa: E402
from _clouds import dense                                                # noqa: E402
from test_gpu_d1d2_exact import D2_CASES, _dist2, _plane                 # noqa: E402

# source points, source colours, target points, target colours
COLOR_CASES = {
    "dense_res12": dense(1, 12, 700) + dense(2, 12, 500),
    "dense_res20": dense(3, 20, 1500) + dense(4, 20, 2500),
    "dense_ties": dense(1, 12, 700) + (dense(2, 12, 500)[0][::-1].copy(), dense(2, 12, 500)[1]),
}
OFFSET = np.array([2048 - 20, 5, 4096 - 20], np.int64)       # the reference depends on differences of coordinates only


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= 1e-12 * np.abs(want)))


def test_offsets_follow_the_documented_order():
    off, d2 = gref.offsets(9)
    assert len(off) == 123 and off[0].tolist() == [0, 0, 0] and np.array_equal(d2, (off * off).sum(1))
    assert off[1:7].tolist() == [[-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 1, 0], [1, 0, 0]]
    key = list(zip(d2.tolist(), off[:, 0].tolist(), off[:, 1].tolist(), (-off[:, 2]).tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)


@pytest.mark.parametrize("name", sorted(D2_CASES))
def test_d1_d2_against_brute_force(name):
    a, na, b, _ = D2_CASES[name]
    d = _dist2(a, b)
    tie_ab, tie_ba = d == d.min(1, keepdims=True), (d == d.min(0, keepdims=True)).T
    for shift in (0, OFFSET):
        ab, ba = gref.tied(a + shift, b + shift), gref.tied(b + shift, a + shift)
        assert np.array_equal(ab.best, d.min(1)) and np.array_equal(ba.best, d.min(0))
        assert np.array_equal(ab.count, tie_ab.sum(1)) and np.array_equal(ba.count, tie_ba.sum(1))
        pairs = np.zeros(d.shape, bool)
        pairs[ab.qi, ab.tj] = True
        assert np.array_equal(pairs, tie_ab) and len(ab.qi) == int(tie_ab.sum())
        assert np.all(np.diff(ab.qi) >= 0)
        for td, near in ((ab, d.min(1)), (ba, d.min(0))):
            assert gref.d1(td) == (float(np.float64(int(near.sum())) / np.float64(len(near))), float(near.max()))
        # the transferred normals: the integer rule as test_d2_ties_against_brute_force restates it
        fixed = np.rint(na.astype(np.float64) * 2.0 ** 40).astype(np.int64)
        sums, count = tie_ab.T.astype(np.int64) @ fixed, tie_ab.sum(0)
        want_nb = np.where(count[:, None] > 0, sums.astype(np.float64) / 2.0 ** 40 / np.maximum(count, 1)[:, None], 0.0).astype(np.float32)
        nb = gref.transfer_normals(ab, na)
        assert nb.dtype == np.float32 and nb.tobytes() == want_nb.tobytes()
        p_ab, p_ba = _plane(a, b, want_nb, tie_ab), _plane(b, a, na, tie_ba)
        assert _close(gref.plane(ab, a + shift, b + shift, nb), p_ab) and _close(gref.plane(ba, b + shift, a + shift, na), p_ba)
        assert _close(gref.d2(ab, a + shift, b + shift, nb), (p_ab.mean(), p_ab.max()))
        assert _close(gref.d2(ba, b + shift, a + shift, na), (p_ba.mean(), p_ba.max()))


@pytest.mark.parametrize("name", sorted(COLOR_CASES))
def test_colours_against_the_numpy_rule(name):
    s, cs, t, ct = COLOR_CASES[name]
    want_c, want_n = cref.recolor(s, cs, t)
    st, ts = gref.tied(s + OFFSET, t + OFFSET), gref.tied(t + OFFSET, s + OFFSET)
    got_c, got_n = gref.recolor(st, ts, cs)
    assert got_c.dtype == np.uint8 and got_n.dtype == np.int32
    assert np.array_equal(got_n, want_n) and np.array_equal(got_c, want_c)
    assert (want_n == 0).any() and (want_n > 1).any()                   # both branches of the rule
    assert _close(gref.color_mse(st, cs, ct), cref.color_mse(s, cs, t, ct))
    assert _close(gref.color_mse(ts, ct, cs), cref.color_mse(t, ct, s, cs))


def test_the_reference_refuses_what_the_gpu_tests_must_not_launch():
    a = np.array([[0, 0, 0], [5, 5, 5]])
    with pytest.raises(AssertionError, match="no target within"):
        gref.tied(a, a[:1])                                              # (5, 5, 5) is 75 > 9 from its target
    with pytest.raises(AssertionError, match="dense block"):
        gref.tied(a, a + 200)
    assert gref.tied(a, a[:1], max_d2=75).best.tolist() == [0, 75]
