"""-m gpu: the rate and loss reverse kernels of csrc/train.hip, each called directly and checked element by element.

    laplace_bwd_kernel                                   pcgc_laplace_likelihood_bwd, _dev
    factorized_bwd_kernel + factorized_bwd_final_kernel  pcgc_factorized_likelihood_bwd, _dev
    bce_bwd_kernel                                       pcgc_bce_bwd, _dev
    abs_max_fwd_kernel / abs_max_bwd_kernel              pcgc_abs_max
    relu_bwd_kernel                                      pcgc_relu_bwd

The reference (tests/_loss_grad_ref.py) is torch autograd over the oracle's own forward functions in float64; the limit of
every bounded check is the distance of the SAME autograd in float32 on the CPU from float64, bin by bin:
E(kernel) <= 4 * E(float32 CPU) + 16 * 2^-24 (the rule and its reasons are in the reference's docstring).  The selections
(abs_max, relu_bwd) and every statement about zeros, twins and repeated calls are bit-exact.

E pairs measured on an MI355X, (kernel, float32 CPU autograd), each against float64:

  Laplace, p64 in      [1e-2, 1]           [1e-4, 1e-2)        [1e-6, 1e-4)        [1e-8, 1e-6)
  typical  dy        7.7e-06, 7.7e-06    0.00022, 0.00022    0.0087, 0.0087      0.99, 0.99
  typical  dscale    1.6e-05, 1.6e-05    0.00022, 0.00022    0.0087, 0.0087      0.99, 0.99
  wide     dy        0.00013, 0.00013    3.4e-06, 4.6e-06
  wide     dscale    0.00085, 0.00085    0.00026, 0.0002
  flip     dy        1.7e-05, 1.7e-05    0.00056, 0.00056    0.056, 0.056        1, 1
  flip     dscale    0.0013, 0.0013      0.00056, 0.00056    0.056, 0.056        1, 1
  tail     dy        2.5e-07, 3.4e-07    2.6e-07, 3.2e-07    2.6e-07, 3.2e-07    2.5e-07, 3.2e-07
  tail     dscale    3.7e-06, 2.9e-06    6.9e-07, 5.7e-07    5.8e-07, 5.9e-07    5.5e-07, 4.4e-07

  BCE, factor in       [1e-1, 1]  [1e-2, 1e-1)  ...  [1e-7, 1e-6)
  empty (o)         1.6e-07, 2.3e-07; 1.6e-07, 1.6e-07; 1.6e-07, 1.5e-07; 1.4e-07, 1.4e-07; 1.4e-07, 1.4e-07; 1.4e-07, 1.4e-07; 1.4e-07, 1.5e-07
  occupied (1 - o)  7.5e-07, 7.4e-07; 8.1e-06, 8.1e-06; 8.5e-05, 8.5e-05; 0.00068, 0.00068; 0.0058, 0.0058; 0.058, 0.058; 0.2, 0.2
  pred = +-16.0     pred=16 label=0: 8.2e-09, 8.2e-09; pred=-16 label=0: 7.4e-08, 3.6e-08; pred=16 label=1: 0.059, 0.059; pred=-16 label=1: 3e-08, 5.2e-08

  factorized, worst of the four cases of each C      dz                    the twelve parameter tensors
  C = 1                                            0.0022, 0.0026        1.8e-05, 0.00014
  C = 8                                            0.002, 0.0016         7.7e-06, 1.3e-05
  C = 16                                           0.0016, 0.0019        9.1e-06, 1.2e-05
  C = 32                                           0.002, 0.0015         1e-05, 7.2e-06
  C = 64                                           0.002, 0.0016         6e-06, 6.4e-06
  C = 128                                          0.0019, 0.0016        1.7e-05, 1.3e-05
  C = 256                                          0.0019, 0.0019        1e-05, 7.7e-06

Of the 410 bins the closest came to 0.49 of its limit.  pytest -s prints every pair.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _loss_grad_ref as R                     # noqa: E402
from pcgcv1_amd import _lib                    # noqa: E402

F32 = torch.float32
N1 = 4246.0                                    # occupied voxels of a typical cube: the step's coefficient is -1 / (ln 2 * n1)
STEP_COEF = np.float32(-1.0 / (R.LN2 * N1))
LAPLACE_COEF = {"typical": STEP_COEF, "wide": np.float32(0.75), "flip": np.float32(-1.3), "tail": np.float32(0.011)}


def _lib_dev():
    return _lib.hip(), _lib.require_gpu()


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(n, dev, dtype=torch.float32):
    return torch.full((n,), float("nan"), dtype=dtype, device=dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _sums4(dev, n0=900, n1=124):
    """A device double[4] = {s0, n0, s1, n1} as pcgc_bce_sums leaves it."""
    lib = _lib.hip()
    n = n0 + n1
    pred = _up(np.linspace(-3, 3, n).astype(np.float32), dev)
    label = _up((np.arange(n) >= n0).astype(np.float32), dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.pcgc_bce_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.pcgc_bce_sums(_lib.dptr(pred), _lib.dptr(label), n, _lib.dptr(sums), _lib.dptr(ws), ws.numel(), _lib.stream()))
    host = sums.cpu().numpy()
    assert host[1] == n0 and host[3] == n1
    return sums, host


# ------------------------------------------------------------------ Laplace
def _laplace_kernel(y, loc, scale, coef, pad=0, dev_coef=None):
    """-> (dy, dloc, dscale) numpy, each n + pad long (the pad keeps its NaN).  dev_coef = (num, mul, count tensor): the _dev
    entry point."""
    lib, dev = _lib_dev()
    n = int(np.asarray(y).size)
    ty, tl, ts = (_up(v, dev) for v in (y, loc, scale))
    out = [_nan(n + pad, dev) for _ in range(3)]
    if dev_coef is None:
        _lib.check(lib.pcgc_laplace_likelihood_bwd(_lib.dptr(ty), _lib.dptr(tl), _lib.dptr(ts), float(coef), R.BOUND, _lib.dptr(out[0]),
                                                   _lib.dptr(out[1]), _lib.dptr(out[2]), n, _lib.stream()))
    else:
        num, mul, count = dev_coef
        _lib.check(lib.pcgc_laplace_likelihood_bwd_dev(_lib.dptr(ty), _lib.dptr(tl), _lib.dptr(ts), num, mul, _lib.dptr(count), R.BOUND,
                                                       _lib.dptr(out[0]), _lib.dptr(out[1]), _lib.dptr(out[2]), n, _lib.stream()))
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def _laplace_case(regime):
    y, loc, scale, claims = R.gen_laplace(regime)
    coef = LAPLACE_COEF[regime]
    return (y, loc, scale, claims, coef, R.laplace_grad(y, loc, scale, coef), R.laplace_grad(y, loc, scale, coef, F32),
            _laplace_kernel(y, loc, scale, coef))


@pytest.mark.parametrize("regime", R.LAPLACE_REGIMES)
def test_laplace_bwd_matches_float64_autograd_bin_by_bin(regime):
    y, loc, scale, claims, coef, g64, g32, k = _laplace_case(regime)
    assert all(np.isfinite(a).all() for a in k)
    assert np.array_equal(k[1], -k[0])                       # dloc == -dy: equal values are equal bits but for the sign of a zero
    masks = R.bin_masks(g64[3], R.LAPLACE_BINS)
    for b in claims:
        m = masks[b]
        assert int(m.sum()) >= R.MIN_BIN
        for j, name in ((0, "dy"), (2, "dscale")):
            R.compare("laplace %s %s p in [%.0e, %.0e)" % (regime, name, *R.LAPLACE_BINS[b]), k[j][m], g32[j][m], g64[j][m])


@pytest.mark.parametrize("n", [1, 255, 257])
def test_laplace_bwd_small_sizes_equal_the_prefix_of_the_large_run(n):
    """Every element depends on its own inputs alone: the first n of the million-element run (pinned above, grid-stride loop
    on its second trip) bit for bit, and nothing written past n."""
    y, loc, scale, _, coef, _, _, big = _laplace_case("flip")
    k = _laplace_kernel(y[:n], loc[:n], scale[:n], coef, pad=64)
    for a, b in zip(k, big):
        assert _same_bits(a[:n], b[:n]) and np.isnan(a[n:]).all()


@pytest.mark.parametrize("coef", [STEP_COEF, np.float32(2.5)])
def test_laplace_bwd_engineered_elements(coef):
    y, loc, scale = R.engineered_laplace_zero()
    for a in _laplace_kernel(y, loc, scale, coef):
        assert np.all(a == 0), a                             # 2v == loc; p == 0 in either tail; scale at its floor, y far away


@pytest.mark.parametrize("coef", [STEP_COEF, np.float32(2.5)])
def test_laplace_bwd_edge_on_loc_at_the_scale_floor(coef):
    """scale = 1e-9 with y + 0.5 == loc exactly: finite, and the float64 value to 1e-5 relative.  float64 (and float32)
    autograd give 0 in all three outputs with p = 0.5: the gradient of tf.abs is sign(), 0 for the edge that sits on loc, and
    the other edge's exp(-1e9) is 0.  (With the density 1 / (2 scale) = 5e8 counted at that edge dy would be coef * 1e9.)  Then
    the same tie at ordinary scales, where the other edge keeps its density: well-conditioned (p > 0.1, float32 autograd is
    within 1e-6 of float64), so the same 1e-5."""
    y, loc, scale = R.engineered_laplace_edge()
    k, g64 = _laplace_kernel(y, loc, scale, coef), R.laplace_grad(y, loc, scale, coef)
    for a, g in zip(k, g64[:3]):
        assert np.isfinite(a).all() and np.all(np.abs(a - g) <= 1e-5 * np.abs(g)), (a, g)
    y, loc, scale = R.engineered_laplace_edge_wide()
    k, g64 = _laplace_kernel(y, loc, scale, coef), R.laplace_grad(y, loc, scale, coef)
    for a, g in zip(k, g64[:3]):
        assert np.all(g != 0) and np.all(np.abs(a - g) <= 1e-5 * np.abs(g)), (a, g)


def test_laplace_bwd_dev_equals_its_host_twin():
    lib, dev = _lib_dev()
    y, loc, scale = (v[:70001] for v in _laplace_case("flip")[:3])
    sums, host = _sums4(dev)
    num, mul = 0.37, -R.LN2
    a = _laplace_kernel(y, loc, scale, np.float32(num / (mul * host[3])))
    b = _laplace_kernel(y, loc, scale, None, dev_coef=(num, mul, sums[3:4]))
    assert all(_same_bits(p, q) for p, q in zip(a, b)) and np.abs(a[0]).max() > 0


# ------------------------------------------------------------------ factorized prior
def _fz_kernel(z, params, coef, C, poison=False, dev_coef=None):
    lib, dev = _lib_dev()
    n = int(z.size)
    tz, tp = _up(z, dev), _up(params, dev)
    nbytes = int(lib.pcgc_factorized_bwd_workspace_bytes(C))
    assert nbytes % 4 == 0
    if poison:
        ws, dz, dp = _nan(nbytes // 4, dev), _nan(n, dev), _nan(44 * C, dev)
    else:
        ws, dz, dp = torch.zeros(nbytes // 4, dtype=F32, device=dev), torch.zeros(n, dtype=F32, device=dev), torch.zeros(44 * C, dtype=F32, device=dev)
    if dev_coef is None:
        _lib.check(lib.pcgc_factorized_likelihood_bwd(_lib.dptr(tz), _lib.dptr(tp), float(coef), R.BOUND, _lib.dptr(dz), _lib.dptr(dp), n, C,
                                                      _lib.dptr(ws), nbytes, _lib.stream()))
    else:
        num, mul, count = dev_coef
        _lib.check(lib.pcgc_factorized_likelihood_bwd_dev(_lib.dptr(tz), _lib.dptr(tp), num, mul, _lib.dptr(count), R.BOUND, _lib.dptr(dz),
                                                          _lib.dptr(dp), n, C, _lib.dptr(ws), nbytes, _lib.stream()))
    torch.cuda.synchronize()
    return dz.cpu().numpy(), dp.cpu().numpy()


@pytest.mark.parametrize("C", R.FZ_CHANNELS)
def test_factorized_bwd_matches_float64_autograd(C):
    """C = 1: six butterfly steps; 64: none; 128, 256: the LDS reduction; 8, 16, 32: the trainers' channel counts.

    dz is one bin per case: the inputs never fill all eight decades of p64 down to 1e-8 (the factorized tails are wide, few
    elements lie below 1e-5), and a maximum over a few dozen elements is no measure of anything.  For the same reason the
    m = 1 case, n = C elements in all, is sixteen draws, each its own call, judged together as one bin."""
    for kind, pert in R.FZ_KINDS:
        w = R.eb_weights(C, pert)
        params = R.pack_params(w)
        coef = np.float32(0.5) if kind == "trip" and pert else STEP_COEF
        m = R.fz_m(C, kind)
        tag = "factorized C=%d m=%d %s" % (C, m, "perturbed" if pert else "raw")
        dzs, ep = [], {}
        for draw in range(R.FZ_DRAWS_ONE if m == 1 else 1):
            z, _ = R.gen_factorized(C, m, w, seed=draw)
            dz64, dp64, p64 = R.factorized_grad(z, w, coef)
            dz32, dp32, _ = R.factorized_grad(z, w, coef, F32)
            dz, dp = _fz_kernel(z, params, coef, C)
            assert np.isfinite(dz).all() and np.isfinite(dp).all()
            assert np.all(dz[p64 < R.BOUND / 2] == 0)        # below the floor (the +-1000 among them): no gradient, no weight
            dzs.append((dz, dz32, dz64))
            k, g32, g64 = R.unpack_params(dp, C), R.unpack_params(dp32, C), R.unpack_params(dp64, C)
            for name in g64:                                 # each tensor on its own largest |g64|, the worst draw counts
                ep[name] = np.maximum(ep.get(name, 0.0), R.err_pair(k[name], g32[name], g64[name], param=True))
            # nothing is read before it is written and the sums run in a fixed order
            dz2, dp2 = _fz_kernel(z, params, coef, C, poison=True)
            assert _same_bits(dz, dz2) and _same_bits(dp, dp2), tag
        R.compare(tag + " dz", *(np.concatenate(v) for v in zip(*dzs)))
        for name, (ek, e32) in ep.items():
            R.judge("%s d%s" % (tag, name[10:]), len(dzs) * g64[name].size, ek, e32)


def test_factorized_bwd_dev_equals_its_host_twin():
    lib, dev = _lib_dev()
    C = 8
    w = R.eb_weights(C, True)
    z, _ = R.gen_factorized(C, 1000, w)
    sums, host = _sums4(dev)
    num, mul = 1.0, -R.LN2
    a = _fz_kernel(z, R.pack_params(w), np.float32(num / (mul * host[3])), C)
    b = _fz_kernel(z, R.pack_params(w), None, C, poison=True, dev_coef=(num, mul, sums[3:4]))
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and np.abs(a[1]).max() > 0


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_factorized_bwd_refuses_what_it_cannot_run(entry):
    lib, dev = _lib_dev()
    sums, _ = _sums4(dev)

    def call(C, n, short=0):
        tz, tp = torch.zeros(max(n, 1), dtype=F32, device=dev), torch.zeros(44 * max(C, 1), dtype=F32, device=dev)
        dz, dp = torch.full((max(n, 1),), 7.0, device=dev), torch.full((44 * max(C, 1),), 7.0, device=dev)
        nbytes = int(lib.pcgc_factorized_bwd_workspace_bytes(C))
        ws = torch.full((nbytes,), 7, dtype=torch.uint8, device=dev)
        if entry == "host":
            rc = lib.pcgc_factorized_likelihood_bwd(_lib.dptr(tz), _lib.dptr(tp), -1.0, R.BOUND, _lib.dptr(dz), _lib.dptr(dp), n, C,
                                                    _lib.dptr(ws), nbytes - short, _lib.stream())
        else:
            rc = lib.pcgc_factorized_likelihood_bwd_dev(_lib.dptr(tz), _lib.dptr(tp), 1.0, -R.LN2, _lib.dptr(sums[3:4]), R.BOUND,
                                                        _lib.dptr(dz), _lib.dptr(dp), n, C, _lib.dptr(ws), nbytes - short, _lib.stream())
        torch.cuda.synchronize()
        msg = lib.pcgc_last_error().decode()
        untouched = bool((dz == 7.0).all()) and bool((dp == 7.0).all()) and bool((ws == 7).all())
        return rc, msg, untouched

    assert call(8, 64)[0] == 0
    for args in ((3, 30), (8, 60), (8, 64, 1)):              # C does not divide 256; n no multiple of C; workspace a byte short
        rc, msg, untouched = call(*args)
        assert rc != 0 and "pcgc_factorized_likelihood_bwd" in msg and untouched, (args, rc, msg)


# ------------------------------------------------------------------ BCE
def _bce_kernel(pred, label, c0, c1, pad=0, dev_coef=None):
    lib, dev = _lib_dev()
    n = int(pred.size)
    tp, tl = _up(pred, dev), _up(label, dev)
    out = _nan(n + pad, dev)
    if dev_coef is None:
        _lib.check(lib.pcgc_bce_bwd(_lib.dptr(tp), _lib.dptr(tl), float(c0), float(c1), _lib.dptr(out), n, _lib.stream()))
    else:
        sums, a0, a1 = dev_coef
        _lib.check(lib.pcgc_bce_bwd_dev(_lib.dptr(tp), _lib.dptr(tl), _lib.dptr(sums), a0, a1, _lib.dptr(out), n, _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


BCE_C = (np.float32(0.75 * 3.0 / 258000.0), np.float32(0.75 / N1))          # alpha * beta / n0, alpha / n1 of a 64^3 cube


@functools.lru_cache(maxsize=None)
def _bce_case():
    pred, label = R.gen_bce()
    c0, c1 = BCE_C
    return pred, label, R.bce_grad(pred, label, c0, c1)[0], R.bce_grad(pred, label, c0, c1, F32)[0], _bce_kernel(pred, label, c0, c1)


def test_bce_bwd_matches_float64_autograd_bin_by_bin():
    pred, label, g64, g32, k = _bce_case()
    assert np.isfinite(k).all() and np.all(k[label < 0] == 0)
    f = R.bce_factor(pred, label)
    for (lo, hi), m in zip(R.BCE_BINS, R.bin_masks(f, R.BCE_BINS)):
        for cls, sel in (("empty, o", label == 0), ("occupied, 1 - o", label > 0)):
            mm = m & sel
            assert int(mm.sum()) >= R.MIN_BIN
            R.compare("bce %s in [%.0e, %.0e)" % (cls, lo, hi), k[mm], g32[mm], g64[mm])


@pytest.mark.parametrize("n", [1, 255, 257])
def test_bce_bwd_small_sizes_equal_the_prefix_of_the_large_run(n):
    pred, label, _, _, big = _bce_case()
    k = _bce_kernel(pred[:n], label[:n], *BCE_C, pad=64)
    assert _same_bits(k[:n], big[:n]) and np.isnan(k[n:]).all()


def test_bce_bwd_engineered_elements():
    pred, label, inside = R.engineered_bce()
    c0, c1 = BCE_C
    k, g64, g32 = _bce_kernel(pred, label, c0, c1), R.bce_grad(pred, label, c0, c1)[0], R.bce_grad(pred, label, c0, c1, F32)[0]
    assert np.all(k[~inside] == 0) and np.all(k[label < 0] == 0), k          # |pred| >= 17: outside the clip
    for i in np.nonzero(inside & (label >= 0))[0]:                            # +-16.0: inside, the full value
        assert k[i] != 0
        R.compare("bce pred=%g label=%g" % (pred[i], label[i]), k[i:i + 1], g32[i:i + 1], g64[i:i + 1])


def test_bce_bwd_dev_equals_its_host_twin():
    lib, dev = _lib_dev()
    pred, label = (v[:70001] for v in _bce_case()[:2])
    sums, host = _sums4(dev)
    a0, a1 = 0.75 * 3.0, 0.75
    a = _bce_kernel(pred, label, np.float32(a0 / host[1]), np.float32(a1 / host[3]))
    b = _bce_kernel(pred, label, None, None, dev_coef=(sums, a0, a1))
    assert _same_bits(a, b) and np.abs(a).max() > 0


# ------------------------------------------------------------------ selections: bit-exact
@pytest.mark.parametrize("lb", [1e-9, 0.11])
def test_abs_max_both_directions_bit_exact(lb):
    """lb = 1e-9 is the trainer's; at 0.11 the branch is common.  +-0, |s| == lb with both signs (the tie goes to |s|, as in
    TensorFlow) and |s| one ulp either side of lb lead the array; n crosses the grid cap."""
    lib, dev = _lib_dev()
    n = R.N_BIG
    s, dscale, _ = R.gen_abs_max(lb, n)
    ts, td = _up(s, dev), _up(dscale, dev)
    fwd, bwd = _nan(n + 64, dev), _nan(n + 64, dev)
    _lib.check(lib.pcgc_abs_max(_lib.dptr(ts), lb, None, _lib.dptr(fwd), n, _lib.stream()))
    _lib.check(lib.pcgc_abs_max(_lib.dptr(ts), lb, _lib.dptr(td), _lib.dptr(bwd), n, _lib.stream()))
    torch.cuda.synchronize()
    fwd, bwd = fwd.cpu().numpy(), bwd.cpu().numpy()
    assert np.isnan(fwd[n:]).all() and np.isnan(bwd[n:]).all()
    assert _same_bits(fwd[:n], R.abs_max_fwd(s, lb))
    ref = R.abs_max_bwd(dscale, s, lb)
    assert _same_bits(bwd[:n], ref), np.nonzero(_bits(bwd[:n]) != _bits(ref))[0][:8]


@pytest.mark.parametrize("nvox,C,dy_cs,dy_co,with_y", [
    (1031, 8, 16, 0, True), (1031, 8, 16, 8, True), (1031, 8, 8, 0, True), (1031, 8, 16, 8, False), (1, 8, 8, 0, True),
    (4096 * 256 // 8 + 41, 8, 16, 8, True),                  # n = nvox * C crosses the grid cap
])
def test_relu_bwd_bit_exact(nvox, C, dy_cs, dy_co, with_y):
    """A channel slice of dy masked by y > 0 (0.0, -0.0 and negative denormals mask, positive denormals pass); y = NULL copies."""
    lib, dev = _lib_dev()
    dy, y = R.gen_relu(nvox, C, dy_cs)
    n = nvox * C
    td, ty = _up(dy, dev), (_up(y, dev) if with_y else None)
    out = _nan(n + 64, dev)
    _lib.check(lib.pcgc_relu_bwd(_lib.dptr(td), dy_cs, dy_co, _lib.dptr(ty), _lib.dptr(out), nvox, C, _lib.stream()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[n:]).all()
    assert _same_bits(out[:n], R.relu_bwd(dy, dy_cs, dy_co, y if with_y else None, nvox, C))
