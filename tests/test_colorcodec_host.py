"""The colour codec's host side, no GPU: YCoCg-R, the numpy statement of RAHT (tests/_raht_ref.py) against hand-checked cases and
the transform's algebra, the derived distortion bound, the integer tables and the .colors container."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raht_ref as ref                                                  # noqa: E402
from pcgcv1_amd import colorcodec as cc                                  # noqa: E402

STEPS = (1, 2, 4, 8, 16, 32)


def _cloud(seed, res, n):
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def test_ycocg_r_is_reversible_and_in_range():
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    rgb = np.concatenate([corners, np.random.default_rng(0).integers(0, 256, (10 ** 6, 3)).astype(np.uint8)])
    for mod in (cc, ref):
        ycc = mod.rgb_to_ycocg(rgb)
        assert np.array_equal(mod.ycocg_to_rgb(ycc), rgb.astype(np.int32))
        assert ycc[:, 0].min() >= 0 and ycc[:, 0].max() <= 255
        assert ycc[:, 1:].min() >= -255 and ycc[:, 1:].max() <= 255
        assert ycc[:, 1].min() == -255 and ycc[:, 1].max() == 255
    assert np.array_equal(cc.rgb_to_ycocg(rgb), ref.rgb_to_ycocg(rgb))


def test_morton_order_puts_x_on_top():
    p = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [3, 0, 0]])
    assert ref.morton_keys(p, 2).tolist() == [1, 2, 4, 4 + 32]
    assert ref.depth_of(np.array([[0, 0, 0]])) == 0 and ref.depth_of(p) == 2 and ref.depth_of(np.array([[4095, 0, 0]])) == 12


def test_hand_checked_two_and_three_points():
    # weights 1 + 1: lo = (a1 + a2) / sqrt 2, hi = (a2 - a1) / sqrt 2; the pair sits at level 0, the DC is subband 3d = 3
    p = np.array([[0, 0, 1], [0, 0, 0]])
    coef, sub, w = ref.forward(p, np.array([[20, 2, -4], [10, 0, 0]]))
    assert sub.tolist() == [3, 0] and w.tolist() == [2, 2]
    assert np.allclose(coef, [[30 / np.sqrt(2), 2 / np.sqrt(2), -4 / np.sqrt(2)], [10 / np.sqrt(2), 2 / np.sqrt(2), -4 / np.sqrt(2)]], rtol=1e-15)
    # a third point joins at level 1 with weights 2 + 1: swapped square roots would give (sqrt 2 * 40 + 30 / sqrt 2 ...) instead
    p = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0]])
    coef, sub, w = ref.forward(p, np.array([[10, 0, 0], [20, 0, 0], [40, 0, 0]]))
    lo = 30 / np.sqrt(2)
    assert sub.tolist() == [3, 0, 1] and w.tolist() == [3, 2, 3]
    assert np.allclose(coef[:, 0], [(np.sqrt(2) * lo + 40) / np.sqrt(3), 10 / np.sqrt(2), (np.sqrt(2) * 40 - lo) / np.sqrt(3)], rtol=1e-15)
    assert np.allclose(coef[0, 0], 70 / np.sqrt(3)) and np.allclose(coef[2, 0], (np.sqrt(2) * 40 - 30 / np.sqrt(2)) / np.sqrt(3))
    # two points that only meet at the root
    coef, sub, w = ref.forward(np.array([[0, 0, 0], [7, 7, 7]]), np.array([[1, 2, 3], [5, 6, 7]]))
    assert sub.tolist() == [9, 8] and np.allclose(coef[1], [4 / np.sqrt(2)] * 3)
    # one point: its attribute is the DC
    coef, sub, w = ref.forward(np.array([[5, 6, 7]]), np.array([[9, 8, 7]]))
    assert sub.tolist() == [9] and w.tolist() == [1] and coef.tolist() == [[9.0, 8.0, 7.0]]


@pytest.mark.parametrize("seed,res,n", [(1, 12, 700), (2, 32, 3000), (3, 200, 5000), (4, 4096, 2000)])
def test_transform_algebra(seed, res, n):
    p, c = _cloud(seed, res, n)
    a = ref.rgb_to_ycocg(c).astype(np.float64)
    coef, sub, w = ref.forward(p, a)
    m, d = len(p), ref.depth_of(p)
    assert coef.shape == (m, 3) and sub.shape == (m,) and w.shape == (m,)            # exactly M coefficients per channel
    assert sub[0] == 3 * d and w[0] == m and (sub[1:] < 3 * d).all() and (w[1:] >= 2).all()
    e_c, e_a = (coef ** 2).sum(), (a ** 2).sum()
    assert abs(e_c - e_a) <= 1e-10 * e_a
    assert np.abs(ref.inverse(p, coef) - a).max() <= 1e-9
    const = np.tile([[77.0, -3.0, 12.0]], (m, 1))
    flat = ref.forward(p, const)[0]
    assert np.abs(flat[1:]).max() < 1e-9 and np.allclose(flat[0], np.sqrt(m) * const[0])


@pytest.mark.parametrize("step", STEPS)
def test_distortion_bound(step):
    """The transform is orthonormal and |coef - q step| <= step / 2, so the per-channel RMS error in YCoCg before rounding is at
    most step / 2, and after rint (the clip cannot increase it: the true values lie inside the range) at most step / 2 + 1 / 2."""
    p, c = _cloud(10 + step, 64, 20000)
    a = ref.rgb_to_ycocg(c).astype(np.float64)
    dec, q, sub, rec = ref.codec(p, c, step)
    rms = np.sqrt(((rec - a) ** 2).mean(0))
    print(step, "rms before rounding", rms)
    assert (rms <= step / 2 + 1e-9).all()
    rms_int = np.sqrt(((ref.rgb_to_ycocg(dec).astype(np.float64) - a) ** 2).mean(0))
    ycc = np.rint(rec)
    ycc = np.stack([np.clip(ycc[:, 0], 0, 255), np.clip(ycc[:, 1], -255, 255), np.clip(ycc[:, 2], -255, 255)], -1)
    rms_round = np.sqrt(((ycc - a) ** 2).mean(0))
    print(step, "rms after rint + clip", rms_round, "of the decoded rgb in YCoCg", rms_int)
    assert (rms_round <= step / 2 + 0.5 + 1e-9).all()
    if step == 1:                                     # every coefficient within 1/2: the colours survive almost untouched
        assert np.abs(dec.astype(int) - c.astype(int)).max() <= 3


def test_tables_are_integer_built_and_complete():
    for amax, ratios in ((0, [1, 65535, 30000]), (1, [1, 2, 3]), (7, [40000, 65535, 1]), (300, [60000, 65000, 20000]), (cc.AMAX_CAP, [65535, 1, 64000])):
        cdf = cc.build_tables(amax, ratios)
        again = cc.build_tables(amax, list(ratios))
        assert cdf.dtype == np.int32 and cdf.shape == (3, 2 * amax + 3) and cdf.tobytes() == again.tobytes()
        assert (cdf[:, 0] == 0).all() and (cdf[:, -1] == 65536).all()
        assert (np.diff(cdf, axis=1) >= 1).all()                                     # no zero-width symbol
        freq = np.diff(cdf, axis=1)
        assert (freq[:, amax] == freq[:, :-1].max(1)).all()                          # q = 0 is the mode of the values
        assert np.array_equal(freq[:, :amax], freq[:, 2 * amax:amax:-1])             # two-sided
    with pytest.raises(ValueError):
        cc.build_tables(cc.AMAX_CAP + 1, [5])
    with pytest.raises(ValueError):
        cc.build_tables(3, [0])
    assert 1 <= cc.choose_ratio(np.array([10, 0, 0])) <= 65535 and cc.choose_ratio(np.array([1, 5, 9, 30])) > cc.choose_ratio(np.array([30, 9, 5, 1]))


def _host_symbols(p, c, step):
    """what the device hands to the container, from the numpy reference"""
    _, q, sub, _ = ref.codec(p, c, step)
    d = ref.depth_of(p)
    counts = np.bincount(sub, minlength=3 * d + 1)
    qg = q[ref.subband_order(sub)]
    n_coded = cc.coded_levels(counts)
    k = int(counts[:n_coded].sum())
    lev = np.repeat(np.arange(n_coded), counts[:n_coded])
    return d, counts, qg, k, lev


def test_container_round_trip_and_refusals():
    p, c = _cloud(5, 40, 6000)
    d, counts, qg, k, lev = _host_symbols(p, c, 2)
    m = len(p)
    # a small cap on the alphabet of every level so that the escape path is used too
    amax = np.array([min(3, np.abs(qg[:k][lev == l]).max(initial=0)) for l in range(len(set(lev)))], np.int32)
    a = amax[lev][:, None]
    inside = np.abs(qg[:k]) <= a
    sym = np.where(inside, qg[:k] + a, 2 * a + 1).astype(np.int16)
    pos = np.flatnonzero(~inside.reshape(-1))
    assert len(pos) > 100
    data = cc.pack(d, m, 2.0, counts, amax, sym, qg[k:], pos, qg[:k].reshape(-1)[pos])
    assert data == cc.pack(d, m, 2.0, counts, amax, sym, qg[k:], pos, qg[:k].reshape(-1)[pos])          # deterministic
    qstep, amax2, sym2, patch = cc.unpack(data, d, m, counts)
    assert qstep == 2.0 and np.array_equal(amax2, amax) and np.array_equal(sym2, sym)
    q2 = np.zeros_like(qg)
    q2[:k] = sym2.astype(np.int32) - a
    q2.reshape(-1)[patch[:, 0]] = patch[:, 1]
    assert np.array_equal(q2, qg)
    assert cc.header_bytes(data) == cc.HEADER_BYTES + cc.LEVEL_BYTES * len(amax)
    with pytest.raises(ValueError, match="magic"):
        cc.unpack(b"XXXX" + data[4:], d, m, counts)
    with pytest.raises(ValueError, match="version"):
        cc.unpack(data[:4] + b"\x07" + data[5:], d, m, counts)
    with pytest.raises(ValueError, match="M = %d" % m):
        cc.unpack(data, d, m + 1, counts)
    with pytest.raises(ValueError, match="other geometry"):
        cc.unpack(data, d + 1, m, counts)
    other = counts.copy()
    other[0] -= 1
    other[1] += 1
    with pytest.raises(ValueError, match="other geometry"):             # same d and M, another tree
        cc.unpack(data, d, m, other)
    for cut in (10, cc.HEADER_BYTES + 5, len(data) // 2, len(data) - 1):
        with pytest.raises(ValueError, match="truncated"):
            cc.unpack(data[:cut], d, m, counts)
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    with pytest.raises(ValueError, match="checksum"):
        cc.unpack(bytes(flipped), d, m, counts)
    with pytest.raises(ValueError):
        cc.pack(d, m, 2.0, counts, amax, sym[:-1], qg[k:])
    assert struct.unpack("<d", data[16:24])[0] == 2.0 and data[:4] == b"PCRA"


def test_tiny_clouds_are_all_raw():
    p = np.array([[1, 2, 3], [1, 2, 2], [0, 0, 0]])
    c = np.array([[255, 0, 7], [3, 200, 9], [90, 90, 90]], np.uint8)
    d, counts, qg, k, lev = _host_symbols(p, c, 1)
    assert k == 0 and cc.coded_levels(counts) == 0
    data = cc.pack(d, 3, 1.0, counts, [], np.zeros((0, 3), np.int16), qg)
    _, amax, sym, patch = cc.unpack(data, d, 3, counts)
    assert len(amax) == 0 and len(sym) == 0 and np.array_equal(patch[:, 1].reshape(-1, 3), qg)
