"""The colour rate control's device-side numbers in numpy ("rate control"): what pcgc_raht_rate_sweep and
pcgc_color_sse6 must give, integer for integer, and the size estimate in plain Python.  The coefficients are tests/_raht_ref.py's.
"""
import math

import numpy as np

import _raht_ref as ref

RAW_LEAVES = 48            # colorcodec.RAW_LEAVES
ABS_CAP = 2048             # AMAX_CAP + 1: an escaped value counts as this
BINS = 37                  # subbands 0 .. 35 and the DC


def coded_levels(counts):
    """the lowest level above which (itself included) at most RAW_LEAVES leaves remain; the levels below it are coded"""
    counts = [int(c) for c in counts]
    above, l = counts[-1], len(counts) - 1
    while l > 0 and above + counts[l - 1] <= RAW_LEAVES:
        l -= 1
        above += counts[l]
    return l


def level_counts(subband, d):
    return np.bincount(subband, minlength=3 * d + 1).astype(np.int64)


def sweep(points, colors, steps):
    """-> (abs_sums int64 [K, 37, 3], max_abs int32 [K, 37]): per step, coded subband and channel the sum of min(|q|, 2048) with
    q = rint(coef / step), and per step and coded subband the largest |q|; the raw levels and the DC stay 0"""
    points = np.asarray(points)
    d = ref.depth_of(points)
    coef, subband, _ = ref.forward(points, ref.rgb_to_ycocg(colors), d)
    n_coded = coded_levels(level_counts(subband, d))
    sums = np.zeros((len(steps), BINS, 3), np.int64)
    tops = np.zeros((len(steps), BINS), np.int32)
    for k, step in enumerate(steps):
        a = np.abs(ref.quantize(coef, step).astype(np.int64))
        for l in range(n_coded):
            rows = a[subband == l]
            if len(rows):
                sums[k, l] = np.minimum(rows, ABS_CAP).sum(0)
                tops[k, l] = rows.max()
    return sums, tops


def sse6(a, b):
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    r, g, bl = d[:, 0], d[:, 1], d[:, 2]
    return np.array([(r * r).sum(), (g * g).sum(), (bl * bl).sum(), (r * g).sum(), (r * bl).sum(), (g * bl).sum()], np.int64)


def ratio(abs_sum, n):
    """the Q16 ratio of the two-sided geometric table fitted to n values whose magnitudes add up to abs_sum (E|q| = 2r / (1 - r^2))"""
    mean = abs_sum / n if n else 0.0
    r = (math.sqrt(1.0 + mean * mean) - 1.0) / mean if mean > 0 else 0.0
    return min(65535, max(1, int(round(r * 65536))))


def subband_bits(abs_sum, n):
    if n == 0:
        return 0.0
    r = ratio(abs_sum, n) / 65536.0
    return n * -math.log2((1.0 - r) / (1.0 + r)) + abs_sum * -math.log2(r)


def estimate_bytes(counts, sums, coder="range", lanes=64, steps_per_chunk=2048, min_symbols=16384):
    """one step's sums int [37, 3] -> bytes: 36 header, 12 (14) per level row, the levels' bits rounded up to bytes, 3 per raw value,
    and for a rANS level (version 2, at least min_symbols symbols) 4 per chunk and 4 per final state"""
    counts = [int(c) for c in counts]
    n_coded = coded_levels(counts)
    total = 36 + (14 if coder == "rans" else 12) * n_coded + 3 * 3 * sum(counts[n_coded:])
    for l in range(n_coded):
        total += math.ceil(sum(subband_bits(int(sums[l][c]), counts[l]) for c in range(3)) / 8.0)
        n = 3 * counts[l]
        if coder == "rans" and n >= min_symbols:
            per = lanes * steps_per_chunk
            chunks = -(-n // per)
            total += 4 * chunks + 4 * sum(min(lanes, min(per, n - per * i)) for i in range(chunks))
    return total
