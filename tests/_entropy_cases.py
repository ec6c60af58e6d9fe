"""Seeded inputs of the entropy-kernel tests (test_gpu_entropy_forms.py, test_entropy_cases_host.py) and the CPU oracle's
results on them.  Everything here is numpy and oracle/: no GPU, no product code.  Arrays are computed once, shared among the
tests and read-only.

Laplace CDF launches (cdf_case / cdf_reference), one per ncols of CDF_NCOLS, SEG_ROWS rows per segment, segments in this order:
  full width N = ncols, centred:   [-(ncols // 2), -(ncols // 2) + ncols - 1]
  full width, one-sided:           [0, ncols - 1] where that stays <= 16 (ncols <= 17), else pushed against 16: [17 - ncols, 16]
  width 2:                         [-1, 0]
  middle width ncols // 2 + 1:     centred like the first
  width 1:                         [0, 0]  — a constant cube; the only width narrower than ncols = 2
(a range that an earlier segment of the launch already has is not repeated).  All ranges lie inside [-16, 16].
ROWWISE is one more launch: 1000 rows with seg_rows = 1, every row its own segment of a width between 2 and 8, ncols = 8.

Rows, per block of SEG_ROWS (the recipe of test_gpu_parity.py::test_laplace_cdf_integer_algorithm_bit_exact):
  0..5       scale 1e-9, 1e-4, 0.3, 7, 100, 1e4
  6..11      loc 0, 0.5, -0.5, 1, 2, -3: symmetric about a symbol or between two
  16..111    loc = 0 exactly            } mirror-symmetric pmfs where the range is symmetric about loc (about 0; about an axis
  112..207   loc = the range's own axis } that is not positive): the two tails have identical key sequences, every step ties
  208..399   loc from {+-0.5, +-1, 1e-4, -3e-5, 0.013, 0.03}: nearly symmetric, leaders alternate      (16..399: scale in [0.05, 30])
  400..591   loc in +-0.05, scale in [0.1, 0.2]: the heavy rows of the bench operating point
  the rest   loc = 2 * standard normal, scale log-uniform in [1e-3, 60]
Slow rows — deficit 65536 - sum(max(1, rint(pmf * 65536))) above SLOW_DEFICIT, one step of the oracle's quantiser per count —
are capped at SLOW_CAP per block: the first SLOW_CAP stay, the others are drawn again (scale log-uniform in [1e-3, 60]; loc
uniform over the range, except that rows 16..591 keep theirs as long as a scale can be found) until they are not slow.
"""
import functools

import numpy as np

from oracle import entropy as oent

F32 = np.float32
BOUND = 1e-9                               # likelihood_bound of every call
CDF_NCOLS = (2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
ROWWISE = "rowwise"
SEG_ROWS = 1024
SLOW_DEFICIT, SLOW_CAP = 20000, 32
SYM_BLOCK = 192                            # rows per kind in 16..591 (the two symmetric kinds share one)


def cdf_instantiation(ncols):
    """MAXN of the laplace_cdf_kernel<MAXN> that pcgc_laplace_cdf (csrc/entropy.hip) launches for this ncols:
    ncols <= 4 -> <4>, <= 8 -> <8>, <= 16 -> <16>, else <32>."""
    assert 1 <= ncols <= 32
    return 4 if ncols <= 4 else 8 if ncols <= 8 else 16 if ncols <= 16 else 32


def cdf_segments(ncols):
    """[(min, max)] of the launch's segments, in launch order."""
    centred = lambda w: (-(w // 2), -(w // 2) + w - 1)                                                       # noqa: E731
    segs = [centred(ncols), (0, ncols - 1) if ncols - 1 <= 16 else (17 - ncols, 16), (-1, 0), centred(ncols // 2 + 1), (0, 0)]
    out = []
    for s in segs:
        if s not in out:
            out.append(s)
    assert all(-16 <= a <= b <= 16 and b - a + 1 <= ncols for a, b in out)
    return out


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _groups(mn, mx):
    """((min, max), row indices) for every distinct range among the rows."""
    key = mn.astype(np.int64) * 64 + mx
    return [((int(mn[i[0]]), int(mx[i[0]])), i) for i in (np.flatnonzero(key == k) for k in np.unique(key))]


def row_pmf_sums(loc, scale, mn, mx):
    """Per row: sum over the range of max(1, rint(pmf * 65536)), the quantiser's starting point (int64)."""
    out = np.empty(loc.size, np.int64)
    for (a, b), i in _groups(mn, mx):
        pmf = oent.sc_pmf(loc[i, None], scale[i, None], a, b, BOUND)[:, 0, :]
        out[i] = np.maximum(1, np.rint(pmf * F32(65536))).astype(np.int64).sum(1)
    return out


def row_deficits(loc, scale, mn, mx):
    return 65536 - row_pmf_sums(loc, scale, mn, mx)


def _rows(rng, mn, mx):
    """loc, scale, symbols of the rows whose ranges are mn[r]..mx[r] (module docstring)."""
    R, k = mn.size, SYM_BLOCK
    loc = (rng.standard_normal(R) * 2.0).astype(F32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(60.0), R)).astype(F32)
    axis = ((mn + mx) * 0.5).astype(F32)
    for s0 in range(0, R, SEG_ROWS):
        assert min(R, s0 + SEG_ROWS) - s0 >= 16 + 3 * k
        scale[s0:s0 + 6] = [1e-9, 1e-4, 0.3, 7.0, 100.0, 1e4]
        loc[s0 + 6:s0 + 12] = [0.0, 0.5, -0.5, 1.0, 2.0, -3.0]
        scale[s0 + 6:s0 + 12] = [0.7, 0.7, 1.3, 0.2, 2.0, 0.9]
        a = s0 + 16
        loc[a:a + k // 2] = 0.0
        loc[a + k // 2:a + k] = axis[a + k // 2:a + k]
        loc[a + k:a + 2 * k] = rng.choice([0.5, -0.5, 1.0, -1.0, 1e-4, -3e-5, 0.013, 0.03], k)
        scale[a:a + 2 * k] = np.exp(rng.uniform(np.log(0.05), np.log(30.0), 2 * k))
        loc[a + 2 * k:a + 3 * k] = rng.uniform(-0.05, 0.05, k)
        scale[a + 2 * k:a + 3 * k] = rng.uniform(0.1, 0.2, k)
    # the cap on slow rows
    slow = row_deficits(loc, scale, mn, mx) > SLOW_DEFICIT
    again = np.concatenate([np.flatnonzero(slow[s0:s0 + SEG_ROWS])[SLOW_CAP:] + s0 for s0 in range(0, R, SEG_ROWS)])
    kind = np.arange(R) % SEG_ROWS
    kind = (kind >= 16) & (kind < 16 + 3 * k)                  # rows whose loc is the point: they first try another scale alone
    for attempt in range(200):
        if again.size == 0:
            break
        move = again if attempt >= 30 else again[~kind[again]]
        loc[move] = rng.uniform(mn[move] - 0.5, mx[move] + 0.5)
        scale[again] = np.exp(rng.uniform(np.log(1e-3), np.log(60.0), again.size))
        again = again[row_deficits(loc[again], scale[again], mn[again], mx[again]) > SLOW_DEFICIT]
    assert again.size == 0
    symbols = rng.integers(mn, mx + 1).astype(F32)
    return loc, scale, symbols


@functools.lru_cache(maxsize=None)
def cdf_case(name):
    """One launch of pcgc_laplace_cdf: dict of loc, scale, symbols (float32 [rows]), seg_min, seg_max (int32 [rows / seg_rows]),
    rows, seg_rows, ncols, and row_min / row_max (the segment's range repeated per row)."""
    if name == ROWWISE:
        rng = np.random.default_rng(4100)
        rows, seg_rows, ncols = 1000, 1, 8
        w = rng.integers(2, 9, rows)
        seg_min = rng.integers(-16, 16 - w + 2).astype(np.int32)
        seg_min[16:16 + SYM_BLOCK] = -(w[16:16 + SYM_BLOCK] // 2)     # the symmetric rows: ranges about 0 or -0.5, where they tie
        seg_max = (seg_min + w - 1).astype(np.int32)
    else:
        ncols = int(name)
        rng = np.random.default_rng(4000 + ncols)
        segs = cdf_segments(ncols)
        rows, seg_rows = len(segs) * SEG_ROWS, SEG_ROWS
        seg_min, seg_max = (np.array(v, np.int32) for v in zip(*segs))
    assert seg_min.min() >= -16 and seg_max.max() <= 16 and int((seg_max - seg_min).max()) + 1 <= ncols
    row_min, row_max = np.repeat(seg_min, seg_rows), np.repeat(seg_max, seg_rows)
    loc, scale, symbols = _rows(rng, row_min, row_max)
    _frozen(loc, scale, symbols, seg_min, seg_max, row_min, row_max)
    return dict(loc=loc, scale=scale, symbols=symbols, seg_min=seg_min, seg_max=seg_max, row_min=row_min, row_max=row_max,
                rows=rows, seg_rows=seg_rows, ncols=ncols)


@functools.lru_cache(maxsize=None)
def cdf_reference(name):
    """The oracle's answer to cdf_case(name): (cdf_lower uint16 [rows, ncols] with 0xFFFF in the columns k >= N of a row,
    lohi uint32 [rows] = ref[k] | (ref[k + 1] - 1) << 16 with k = symbol - min)."""
    c = cdf_case(name)
    cdf = np.full((c["rows"], c["ncols"]), 0xFFFF, np.uint16)
    lohi = np.empty(c["rows"], np.uint32)
    for (a, b), i in _groups(c["row_min"], c["row_max"]):
        ref = oent.sc_get_cdf(c["loc"][i, None], c["scale"][i, None], a, b)[:, 0, :].astype(np.int64)       # [rows, N + 1]
        n = b - a + 1
        assert ref[:, :n].max() <= 0xFFFF and (ref[:, n] == 65536).all()
        cdf[i, :n] = ref[:, :n]
        k = c["symbols"][i].astype(np.int64) - a
        r = np.arange(i.size)
        lohi[i] = (ref[r, k] | ((ref[r, k + 1] - 1) << 16)).astype(np.uint32)
    return _frozen(cdf, lohi)


# ----------------------------------------------------------------------------
# launches past the block caps of the grid-stride kernels (csrc/entropy.hip): one full sweep plus a ragged second one
# ----------------------------------------------------------------------------
RAGGED = 3 * 256 + 5
SMALL = 257
CAP_LAPLACE = 8192 * 256                   # laplace_likelihood_kernel
CAP_FACTORIZED = 4096 * 256                # factorized_likelihood_kernel
CAP_SYMBOLS = 2048 * 256                   # symbols_to_values_kernel
CAP_SYMBOLS_SEG = 4096 * 256               # symbols_to_values_seg_kernel
CAP_SYMBOLS_SEG8 = 4096 * 256 * 8          # symbols_to_values_seg8_kernel, eight symbols per thread
CAP_REPRO = 4096 * 256                     # repro_eval_kernel
FACTORIZED_C = (8, 3, 64)                  # 3 does not divide the sweep, 64 is kMaxFactorizedC
PMF_RANGE = (-15, 15)


def factorized_n(n, C):
    """pcgc_factorized_likelihood takes whole rows of C channels: n rounded up to the next multiple of C (for C = 3 the
    sizes CAP_FACTORIZED + RAGGED and 258 — one more than SMALL)."""
    return -(-n // C) * C


@functools.lru_cache(maxsize=None)
def laplace_inputs(n):
    """y, loc, scale, noise (float32 [n]) in the manner of test_gpu_parity.py::test_entropy_models_vs_oracle."""
    rng = np.random.default_rng(4200 + n % 1000)
    y = (rng.standard_normal(n) * 2).astype(F32)
    y[:6] = [0.5, 1.5, -0.5, 2.5, -0.0, -2.5]                        # round-half-even cases
    loc = (rng.standard_normal(n) * 0.7).astype(F32)
    scale = np.maximum(np.abs(rng.standard_normal(n)) * 0.8, 1e-9).astype(F32)
    loc[6], y[6] = 2.0, 1.0                                          # sign(2q - loc) == 0 quirk
    loc[n - 1], y[n - 1] = 2.0, 1.0                                  # ... and in the last, ragged, element
    noise = (rng.random(n) - 0.5).astype(F32)
    return _frozen(y, loc, scale, noise)


@functools.lru_cache(maxsize=None)
def laplace_reference(n, training):
    y, loc, scale, noise = laplace_inputs(n)
    return _frozen(*oent.sc_call(y, loc, scale, training=training, noise=noise if training else None, likelihood_bound=BOUND))


PARAM_NAMES = ["%s_%d" % (k, i) for i in range(4) for k in ("matrix", "bais", "factor")]     # the order pcgc.h documents


@functools.lru_cache(maxsize=None)
def factorized_params(C):
    """eb_init_params perturbed by seeded noise so that no two channels coincide: (dict for the oracle, flat float32 [C * 44])."""
    rng = np.random.default_rng(4300 + C)
    p = oent.eb_init_params(C, rng=rng)
    for k in PARAM_NAMES:
        p[k] = (p[k] + rng.standard_normal(p[k].shape) * (0.3 if k.startswith("matrix") else 0.2)).astype(F32)
        p[k].setflags(write=False)
    flat = np.concatenate([p[k].reshape(-1) for k in PARAM_NAMES])
    assert flat.size == C * 44
    return p, _frozen(flat)


@functools.lru_cache(maxsize=None)
def factorized_inputs(n, C):
    """z, noise (float32 [n / C, C])."""
    assert n % C == 0
    rng = np.random.default_rng(4400 + C + n % 1000)
    z = (rng.standard_normal((n // C, C)) * 2).astype(F32)
    z[0, :min(C, 6)] = [0.5, 1.5, -0.5, 2.5, -0.0, -2.5][:min(C, 6)]
    noise = (rng.random(z.shape) - 0.5).astype(F32)
    return _frozen(z, noise)


@functools.lru_cache(maxsize=None)
def factorized_reference(n, C, training):
    z, noise = factorized_inputs(n, C)
    return _frozen(*oent.eb_call(factorized_params(C)[0], z, training=training, noise=noise if training else None,
                                 likelihood_bound=BOUND))


@functools.lru_cache(maxsize=None)
def factorized_pmf_reference(C):
    return _frozen(oent.eb_pmf(factorized_params(C)[0], PMF_RANGE[0], PMF_RANGE[1], BOUND))


@functools.lru_cache(maxsize=None)
def symbols(n):
    """int16 [n + 8] in [0, 31): the tests view it from element 0 (16-byte aligned on the device) or from element 1."""
    return _frozen(np.random.default_rng(4500).integers(0, 31, n + 8, dtype=np.int16))


def seg_offsets(nseg):
    """One offset per segment, no two neighbours equal, -15 and 0 among them (float32 [nseg])."""
    i = np.arange(nseg)
    o = (np.array([-15, 0, -3, 2, -1, 5, -8])[i % 7] + (i // 7) % 3).astype(F32)
    assert nseg < 2 or (o[0] == -15 and o[1] == 0 and (np.diff(o) != 0).all())
    return o


@functools.lru_cache(maxsize=None)
def repro_inputs(fn, n):
    """Arguments of repro::expf_ (0), logf_ (1), tanhf_ (2), sigmoidf_ (3), softplusf_ (4) in the manner of test_repro_math.py."""
    rng = np.random.default_rng(4600 + fn)
    if fn == 1:
        x = np.concatenate([rng.uniform(1, 2, n // 2), np.exp(rng.uniform(-80, 80, n - n // 2))])
        edge = [1.0, 2.0, 0.5, 1e-30, 3e38]
    elif fn == 2:
        x = np.concatenate([rng.uniform(-12, 12, n // 2), rng.uniform(-0.7, 0.7, n - n // 2)])
        edge = [0.0, -0.0, 0.625, -0.625, 50, -50]
    else:
        x = np.concatenate([rng.uniform(-90, 90, n // 2), rng.uniform(-2, 2, n - n // 2)])
        edge = [0.0, -0.0, -87.0, -88.0, 88.0, 89.0, -1e10, 1e10]
    x = np.ascontiguousarray(x, F32)
    x[:len(edge)] = edge
    x[n - len(edge):] = edge                                         # ... and in the ragged tail
    return _frozen(x)


# ----------------------------------------------------------------------------
# pcgc_round_minmax / pcgc_round_minmax_i16: (seg_len, segments); the last reaches blocks_per_seg = 1024
# ----------------------------------------------------------------------------
MINMAX_CASES = ((1, 1000), (255, 9), (4096, 7), (4097, 7), (65536, 7), (4194304 + 4096, 2))
TIES = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, -0.4)
EQUAL_SEG, HIGH_SEG, LOW_SEG = 2, 1, 3     # all equal; holds +40000; holds -40000 (where there are that many segments)


@functools.lru_cache(maxsize=None)
def minmax_input(seg_len, nseg):
    """float32 [nseg * seg_len]: 3 * standard normal, plus, where a segment has room (seg_len >= 255): TIES from its second
    element on, its minimum in its first element and its maximum in its last; segment EQUAL_SEG is all -7.5 (a tie again),
    segment HIGH_SEG holds +40000 and segment LOW_SEG -40000, beyond int16.  With seg_len = 1 the same values are segments of
    their own."""
    rng = np.random.default_rng(4700 + seg_len % 1000)
    x = (rng.standard_normal(nseg * seg_len) * 3).astype(F32)
    s = x.reshape(nseg, seg_len)
    if seg_len >= 255:
        s[:, 1:1 + len(TIES)] = TIES
        s[:, 0] = -17.5 - np.arange(nseg)
        s[:, -1] = 18.5 + np.arange(nseg)
        if nseg > EQUAL_SEG:
            s[EQUAL_SEG] = -7.5
        s[min(HIGH_SEG, nseg - 1), seg_len // 2] = 40000.0
        s[min(LOW_SEG, nseg - 1), seg_len // 3] = -40000.0
    else:
        x[:len(TIES)] = TIES
        x[20:22] = [40000.0, -40000.0]
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def minmax_reference(seg_len, nseg):
    """(q float32, q int16 clamped, seg_min int32, seg_max int32) by numpy."""
    r = np.rint(minmax_input(seg_len, nseg))
    s = r.reshape(nseg, seg_len)
    return _frozen(r, np.clip(r, -32768, 32767).astype(np.int16), s.min(1).astype(np.int32), s.max(1).astype(np.int32))
