"""The colour rate control's host side, no GPU: the step grid, the target's parsing and its argument errors, the numpy statement of
the sweep (tests/_color_rc_ref.py) and the size estimate built on its sums, and the six sums' way to the Y, U, V errors."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_rc_ref as rcref                                            # noqa: E402
import _raht_ref as ref                                                  # noqa: E402
from pcgcv1_amd import colorcodec as cc                                  # noqa: E402
from pcgcv1_amd import test as cli                                       # noqa: E402


def _cloud(seed, res, n):
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def test_grid_endpoints_and_monotonicity():
    assert (cc.QSTEP_GRID_MIN, cc.QSTEP_GRID_MAX) == (-16, 56)
    steps = [cc.grid_step(j) for j in range(cc.QSTEP_GRID_MIN, cc.QSTEP_GRID_MAX + 1)]
    assert len(steps) == 73 and steps[0] == 0.25 and steps[-1] == 128.0 and cc.grid_step(0) == 1.0 and cc.grid_step(16) == 4.0
    ratios = np.array(steps[1:]) / np.array(steps[:-1])
    assert (ratios > 1).all() and np.allclose(ratios, 2 ** 0.125, rtol=1e-12)
    assert cc.SWEEP_MAX_STEPS == 32 and math.ceil(len(steps) / cc.SWEEP_MAX_STEPS) == 3              # the whole grid in three launches


def test_target_parsing():
    assert cc.parse_target("psnr:38") == ("psnr", 38.0)
    assert cc.parse_target("bpp:0.6") == ("bpp", 0.6)
    assert cc.parse_target("psnr:0") == ("psnr", 0.0)
    for bad in ("38", "psnr", "psnr:", "psnr=38", "ssim:0.9", "bpp:0", "bpp:-1", "bpp:nan", "psnr:inf", "psnr:38dB", ":38", "PSNR:38"):
        with pytest.raises(ValueError, match="color_target"):
            cc.parse_target(bad)


def test_argument_errors_come_from_parse_args(capsys):
    args = cli.parse_args(["compress", "x.ply", "--colors", "raht", "--color_target", "psnr:38"])
    assert args.color_target == "psnr:38" and args.color_qstep == 4.0
    assert cli.parse_args(["compress", "x.ply", "--colors", "raht"]).color_target == ""              # the default: --color_qstep rules
    assert cli.parse_args(["compress", "x.ply", "--colors", "raht", "--color_target", "bpp:0.6", "--color_coder", "rans"]).color_target == "bpp:0.6"
    for argv, word in ((["--colors", "raht", "--color_target", "psnr"], "psnr:<dB>"),                # malformed
                       (["--colors", "raht", "--color_target", "bpp:-2"], "bpp:<bits per point>"),
                       (["--color_target", "psnr:38"], "--colors=raht"),                           # a target without the codec
                       (["--colors", "raht", "--color_target", "psnr:38", "--color_qstep", "8"], "--color_qstep")):      # two masters
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["compress", "x.ply"] + argv)
        assert e.value.code == 2                                          # argparse's own exit for an argument error
        assert word in capsys.readouterr().err, (argv, word)


def test_reference_sweep_and_estimate_on_a_hand_made_case():
    """two coded levels worked by hand: the sweep's rows from the reference's coefficients, and the estimate from those rows"""
    p, c = _cloud(2, 8, 120)
    d = ref.depth_of(p)
    coef, subband, _ = ref.forward(p, ref.rgb_to_ycocg(c), d)
    counts = rcref.level_counts(subband, d)
    n_coded = rcref.coded_levels(counts)
    assert n_coded == cc.coded_levels(counts) and 2 <= n_coded < 3 * d and counts[n_coded:].sum() <= 48 < counts[n_coded - 1:].sum()
    steps = [0.25, 1.0, 4.0, 37.5]
    sums, tops = rcref.sweep(p, c, steps)
    for k, step in enumerate(steps):
        q = np.abs(np.rint(coef / step)).astype(np.int64)
        for l in range(37):
            rows = q[subband == l] if l < n_coded else q[:0]
            assert sums[k, l].tolist() == np.minimum(rows, 2048).sum(0).tolist()
            assert tops[k, l] == (rows.max() if len(rows) else 0)
    assert (sums[:, n_coded:] == 0).all() and (tops[:, n_coded:] == 0).all()
    assert (sums[0].sum() > sums[1].sum() > sums[2].sum() > sums[3].sum())
    for coder in ("range", "rans"):
        est = cc.estimate_bytes(counts, sums, coder)
        assert est.shape == (4,) and (np.diff(est) < 0).all()
        for k in range(len(steps)):
            assert est[k] == rcref.estimate_bytes(counts, sums[k], coder)
    # by hand: one coded level of n = 100 values per channel with sums 300, 50, 0, then 10 raw leaves and the DC
    counts = [100, 10, 0, 1]
    assert cc.coded_levels(counts) == 1
    hand = np.zeros((1, 37, 3), np.int64)
    hand[0, 0] = [300, 50, 0]
    bits = 0.0
    for s in (300, 50, 0):
        mean = s / 100
        r = min(65535, max(1, round((math.sqrt(1 + mean * mean) - 1) / mean * 65536))) / 65536 if s else 1 / 65536
        assert round(r * 65536) == cc.ratio_of_sum(s, 100)
        bits += 100 * -math.log2((1 - r) / (1 + r)) + s * -math.log2(r)
    assert cc.estimate_bytes(counts, hand)[0] == 36 + 12 + math.ceil(bits / 8) + 3 * 3 * 11
    assert cc.estimate_bytes(counts, hand, "rans")[0] == 36 + 14 + math.ceil(bits / 8) + 3 * 3 * 11            # 300 symbols: no rANS level
    big = [6000, 40, 1]                                                   # 18000 symbols: one chunk of 64 lanes
    assert cc.estimate_bytes(big, hand, "rans")[0] - cc.estimate_bytes(big, hand, "range")[0] == 2 + 4 + 4 * 64


def test_estimate_sanity():
    n = 1000
    r = 1 / 65536
    zeros = cc.estimate_bits(0, n)
    assert zeros == n * -math.log2((1 - r) / (1 + r)) and 0 < zeros < 1
    assert cc.estimate_bits(0, 0) == 0 and cc.estimate_bits(np.zeros(3, np.int64), np.zeros(3, np.int64)).tolist() == [0, 0, 0]
    sums = np.array([1, 10, 100, 1000, 5000, 10 ** 5, 2048 * n], np.int64)
    once, twice = cc.estimate_bits(sums, n), cc.estimate_bits(2 * sums, n)
    assert (twice > once).all() and (np.diff(once) > 0).all()             # doubling every |q| doubles the sum
    assert np.array_equal(cc.ratios_of_sums(sums, n), [cc.ratio_of_sum(int(s), n) for s in sums])
    # a two-sided geometric source of ratio 1/2 has E|q| = 4/3 and an entropy of log2(3) + 4/3 = 2.92 bits
    assert abs(cc.estimate_bits(4 * n // 3, n) / n - (math.log2(3) + 4 / 3)) < 0.01


def test_six_sums_give_the_yuv_errors():
    rng = np.random.default_rng(11)
    w = np.array([[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]])
    for m in (1, 65, 5000):
        a, b = rng.integers(0, 256, (m, 3)).astype(np.uint8), rng.integers(0, 256, (m, 3)).astype(np.uint8)
        s = rcref.sse6(a, b)
        d = a.astype(np.float64) - b.astype(np.float64)
        assert s.tolist() == [int((d[:, i] * d[:, k]).sum()) for i, k in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
        direct = (((a.astype(np.float64) / 255) @ w.T - (b.astype(np.float64) / 255) @ w.T) ** 2).mean(0)
        got = cc.yuv_mse(s, m)
        assert np.allclose(got, direct, rtol=1e-12, atol=0), (m, got, direct)
        assert cc.psnr_of_mse(got[0]) == -10 * np.log10(got[0])
    assert cc.yuv_mse(np.zeros(6, np.int64), 7).tolist() == [0, 0, 0] and cc.psnr_of_mse(0.0) == float("inf")
    far = rcref.sse6(np.zeros((3, 3), np.uint8), np.full((3, 3), 255, np.uint8))
    assert far.tolist() == [3 * 255 ** 2] * 6 and abs(cc.yuv_mse(far, 3)[0] - 1.0) < 1e-12      # Y's weights add up to 1


def test_psnr_ceiling_is_the_smallest_luma_error_of_one_point():
    """Y's weights are 1063, 3576 and 361 times 0.0002 and 18 * 1063 - 53 * 361 = 1: one point off by (18, 0, -53) has the smallest
    luma error that is not 0, no difference of two uint8 colours has a smaller one, and the ceiling is that point's PSNR."""
    assert (round(0.2126 / 0.0002), round(0.7152 / 0.0002), round(0.0722 / 0.0002)) == (1063, 3576, 361) and math.gcd(1063, 3576, 361) == 1
    d = np.arange(-255, 256, dtype=np.int64)
    e = np.abs(1063 * d[:, None, None] + 3576 * d[None, :, None] + 361 * d[None, None, :])
    assert e[e > 0].min() == 1 and e[255 + 18, 255, 255 - 53] == 1
    a, b = np.array([[18, 7, 0]], np.uint8), np.array([[0, 7, 53]], np.uint8)
    for m in (1, 20000):
        one = cc.psnr_of_mse(cc.yuv_mse(rcref.sse6(a, b), m)[0])
        assert abs(one - cc.psnr_ceiling(m)) < 1e-6, (m, one, cc.psnr_ceiling(m))
    assert 165 < cc.psnr_ceiling(20000) < 166 and cc.psnr_ceiling(10 ** 6) < 200


def test_a_level_of_zeros_alone_is_read_back():
    """At the grid's coarse end whole levels quantise to 0; the range coder writes such a level in no bytes at all, and the readers
    of both versions have to take that for what it is (they used to refuse it as a stream that does not fit the file)."""
    d = 2
    counts = [60, 50, 49, 0, 0, 0, 1]                                     # 3 d + 1 subbands: three coded levels, the DC raw
    m, n_coded = sum(counts), cc.coded_levels(counts)
    assert n_coded == 3 and 3 * max(counts) < cc.RANS_MIN_SYMBOLS
    k_raw = sum(counts[:n_coded])
    amax = np.array([1, 0, 0], np.int32)
    symbols = np.zeros((k_raw, 3), np.int16)
    symbols[:60] = np.random.default_rng(2).integers(0, 3, (60, 3))       # level 0 has something to say, levels 1 and 2 are zeros
    tail = np.array([[5, -3, 2]])
    v1 = cc.pack(d, m, 128.0, counts, amax, symbols, tail)
    assert [struct.unpack("<I", v1[cc.HEADER_BYTES + cc.LEVEL_BYTES * l + 8:][:4])[0] for l in range(3)][1:] == [0, 0]
    step, a, sym, patch = cc.unpack(v1, d, m, counts)
    assert step == 128.0 and a.tolist() == amax.tolist() and np.array_equal(sym, symbols) and patch[-3:, 1].tolist() == [5, -3, 2]
    rows = [struct.unpack("<HHHHI", v1[cc.HEADER_BYTES + cc.LEVEL_BYTES * l:][:cc.LEVEL_BYTES]) for l in range(3)]
    at = cc.HEADER_BYTES + cc.LEVEL_BYTES * 3
    v2 = cc.assemble_v2(d, m, 128.0, counts, amax, [r[1:4] for r in rows], [v1[at:at + rows[0][4]], b"", b""], [(), (), ()], tail)
    got = cc.unpack_v2(v2, d, m, counts)
    assert got[0] == 128.0 and np.array_equal(got[6], symbols) and np.array_equal(got[7], patch)


def test_targets_are_checked_before_the_device_is_touched():
    p, c = _cloud(1, 8, 50)
    for kw in ({}, {"psnr": 30, "bpp": 1.0}):
        with pytest.raises(ValueError, match="exactly one"):
            cc.encode_colors_target(p, c, **kw)
    with pytest.raises(ValueError, match="coder"):
        cc.encode_colors_target(p, c, psnr=30, coder="huffman")
    with pytest.raises(ValueError, match="positive"):
        cc.encode_colors_target(p, c, bpp=0)
