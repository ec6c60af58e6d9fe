"""The host side of the scan smoothing (pcgcv1_amd/smooth.py): the forms parse_spec accepts and refuses, and the rule in numpy
(tests/_smooth_ref.py) against cases worked out by hand.  No device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _smooth_ref as ref                                                # noqa: E402
from pcgcv1_amd import smooth                                            # noqa: E402


@pytest.mark.parametrize("text, want", [("3", (3.0, 2, 6)), ("3:1", (3.0, 1, 6)), ("2.5:8:3", (2.5, 8, 3)), ("16:2:4194304", (16.0, 2, 1 << 22)),
                                        ("0.5:2:6", (0.5, 2, 6)), ("1e0:3", (1.0, 3, 6))])
def test_parse_spec_accepts(text, want):
    s = smooth.parse_spec(text)
    assert (s.radius, s.iters, s.kmin) == want
    assert smooth.parse_spec(s) is s
    again = smooth.parse_spec(s.text)                          # the text it prints is a spec
    assert (again.radius, again.iters, again.kmin) == want and again.text == s.text


def test_the_text_of_a_spec_is_what_the_summary_line_shows():
    assert smooth.parse_spec("3").text == "3:2:6"
    line = smooth.summary_line({"spec": "3:2:6", "moved": 5, "points": 7, "rms_move": 0.25}, 12, 9)
    assert line == "smooth: 3:2:6 moved 5 of 7 points, rms move 0.2500 voxels; voxels 12 -> 9"


@pytest.mark.parametrize("text", ["", ":", "3:", ":2", "3::6", "0", "-1", "16.5", "nan", "inf", "x", "3:0", "3:9", "3:1.5", "3:two", "3:2:2",
                                  "3:2:4194305", "3:2:6:1", "3,2"])
def test_parse_spec_refuses(text):
    with pytest.raises(ValueError, match="^smooth: "):
        smooth.parse_spec(text)


def test_three_points_by_hand():
    """(0,0,0), (1,0,0), (0,1,0) within 1.5 of each other: the sums in 2^-16 by hand; three points span a plane that holds all
    of them, here z = 0 exactly, so nobody moves although everybody is `moved`"""
    g = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    out, moved, K, S, Q = ref.step(g, 1.5, 3)
    u = 65536
    assert K.tolist() == [3, 3, 3] and moved.tolist() == [1, 1, 1]
    assert S.tolist() == [[u, u, 0], [-2 * u, u, 0], [u, -2 * u, 0]]
    assert Q.tolist() == [[u * u, 0, 0, u * u, 0, 0], [2 * u * u, -u * u, 0, u * u, 0, 0], [u * u, -u * u, 0, 2 * u * u, 0, 0]]
    assert out.tobytes() == g.tobytes()
    # at radius 1.2 the two far points no longer see each other, and with kmin = 3 they stay out
    out, moved, K, _, _ = ref.step(g, 1.2, 3)
    assert K.tolist() == [3, 2, 2] and moved.tolist() == [1, 0, 0] and out.tobytes() == g.tobytes()


def test_a_point_above_a_plane_by_hand():
    """four points on z = 0 around the origin and one 0.5 above it: its covariance is diagonal by symmetry, the normal is the
    z axis, and it moves to the mean height 0.5 / 5; the plane points have K = 4 = kmin - 1 and stay"""
    g = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.5]], np.float32)
    out, moved, K, S, Q = ref.step(g, 1.5, 5)
    assert K.tolist() == [4, 4, 4, 4, 5] and moved.tolist() == [0, 0, 0, 0, 1]
    assert S[4].tolist() == [0, 0, -4 * 32768] and Q[4].tolist() == [2 * 65536 ** 2, 0, 0, 2 * 65536 ** 2, 0, 4 * 32768 ** 2]
    assert out[:4].tobytes() == g[:4].tobytes()
    want = np.float32(0.5 + ((-4 * 32768) / 5.0) / 65536.0)
    assert out[4].tolist() == [0.0, 0.0, float(want)] and abs(float(want) - 0.1) < 1e-7
    # K = kmin: now the plane points move as well, onto the plane fitted to their four neighbours
    assert ref.step(g, 1.5, 4)[1].tolist() == [1, 1, 1, 1, 1]


def test_exactly_coplanar_and_collinear_neighbours_leave_the_bits():
    xy = np.stack(np.meshgrid(np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 2) * 0.75
    plane = np.concatenate([xy, np.full((len(xy), 1), 2.0)], 1).astype(np.float32)
    out, moved, _, _, _ = ref.step(plane, 2.0, 3)
    assert moved.all() and out.tobytes() == plane.tobytes()
    line = np.zeros((9, 3), np.float32)
    line[:, 0] = np.arange(9) * 0.5
    out, moved, _, _, _ = ref.step(line, 2.0, 3)
    assert moved.all() and out.tobytes() == line.tobytes()


def _cloud(seed, n, noise=0.3):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 12, (n, 3))
    p[:, 2] = 5.0 + 0.1 * p[:, 0] + noise * rng.normal(size=n)
    return p.astype(np.float32)


def test_the_sign_of_the_normal_and_the_order_of_the_points_change_no_bit():
    g = _cloud(3, 600)
    out, moved = ref.chain(g, 2.5, 2, 6)
    flipped, moved_f = ref.chain(g, 2.5, 2, 6, negate=True)
    assert moved.sum() > 500 and out.tobytes() == flipped.tobytes() and np.array_equal(moved, moved_f)
    perm = np.random.default_rng(4).permutation(len(g))
    out_p, moved_p = ref.chain(g[perm], 2.5, 2, 6)
    assert out_p.tobytes() == out[perm].tobytes() and np.array_equal(moved_p, moved[perm])


def test_a_noisy_sheet_gets_thinner_and_rows_that_are_not_finite_pass_through():
    g = _cloud(5, 800).astype(np.float64)
    flat = g.copy()
    flat[:, 2] = 5.0 + 0.1 * flat[:, 0]
    g[17] = (np.nan, 1.0, 2.0)
    g[99, 2] = np.inf
    out, moved = ref.scan(g, (-1.0, -1.0, -1.0), 0.5, 5.0, 2, 6)           # voxels of 0.5: a radius of 2.5 units
    assert out[17].tobytes() == g[17].tobytes() and out[99].tobytes() == g[99].tobytes() and not moved[17] and not moved[99]
    ok = np.isfinite(g).all(1)
    before = np.abs(g[ok, 2] - flat[ok, 2]).std()
    after = np.abs(out[ok, 2] - (5.0 + 0.1 * out[ok, 0])).std()
    assert after < 0.5 * before, (before, after)
