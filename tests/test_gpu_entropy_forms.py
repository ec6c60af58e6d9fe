"""-m gpu: the kernels of csrc/entropy.hip in the forms the product launches them, against the CPU oracle and numpy.

test_gpu_parity.py compares these kernels with the oracle at sizes below every launch cap, the Laplace CDF kernel at
ncols = 14 and 31 only (laplace_cdf_kernel<16> and <32>; the committed checkpoints run <4> and <8>) and never its lohi output,
which is all the encoder asks for.  A round trip cannot see a wrong CDF row — encoder and decoder build the same one — so here:
  A  pcgc_laplace_cdf at both ends of every instantiation's ncols interval, cdf_lower and lohi, bit for bit, in the three
     combinations of outputs, with segments narrower than ncols and one launch of one-row segments;
  B  every grid-stride kernel one full sweep past its block cap plus a ragged second sweep, and at n = 257;
  C  pcgc_round_minmax / _i16 with many segments, blocks_per_seg from 1 to the cap of 1024.
Inputs and references: tests/_entropy_cases.py (checked on the CPU by test_entropy_cases_host.py).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _entropy_cases as ec                                               # noqa: E402
from pcgcv1_amd import _lib                                               # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)


def _dev(a):
    return torch.tensor(a).cuda()                                         # a copy: the shared arrays are read-only


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(got, want, what):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r != %r" % (
        what, bad.size, g.size, bad[0], np.asarray(got.cpu() if torch.is_tensor(got) else got).reshape(-1)[bad[0]],
        np.asarray(want).reshape(-1)[bad[0]])


def _ulp_report(got, want, what):
    """Prints and returns (elements whose bits differ, largest distance in units of the reference's last place)."""
    g, w = np.asarray(got.cpu() if torch.is_tensor(got) else got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    ndiff = int((g.view(np.uint32) != w.view(np.uint32)).sum())
    ulps = float((np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)).max())
    print("%s: %d of %d elements differ in bits, largest distance %.3g ulp" % (what, ndiff, g.size, ulps))
    return ndiff, ulps


# ----------------------------------------------------------------------------
# A. pcgc_laplace_cdf
# ----------------------------------------------------------------------------
def _laplace_cdf(c, dev_in, want_cdf, want_lohi):
    """One launch; outputs start as a pattern neither result can hold, so an element the kernel skips shows."""
    rows, ncols = c["rows"], c["ncols"]
    cdf = torch.full((rows, ncols), 0x5A5A, dtype=torch.int16, device="cuda") if want_cdf else None
    lohi = torch.full((rows,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_lohi else None
    loc, scale, mn, mx, sym = dev_in
    _lib.check(_lib.hip().pcgc_laplace_cdf(_lib.dptr(loc), _lib.dptr(scale), _lib.dptr(mn), _lib.dptr(mx), rows, c["seg_rows"], ncols,
                                           ec.BOUND, _lib.dptr(sym) if want_lohi else None, _lib.dptr(cdf), _lib.dptr(lohi),
                                           _lib.stream()), "pcgc_laplace_cdf")
    return (cdf.cpu().numpy().view(np.uint16) if want_cdf else None, lohi.cpu().numpy().view(np.uint32) if want_lohi else None)


def _check_cdf_launch(name):
    c = ec.cdf_case(name)
    ref_cdf, ref_lohi = ec.cdf_reference(name)
    dev_in = [_dev(c[k]) for k in ("loc", "scale", "seg_min", "seg_max", "symbols")]
    both_cdf, both_lohi = _laplace_cdf(c, dev_in, True, True)
    bad = np.flatnonzero((both_cdf != ref_cdf).any(1))
    assert bad.size == 0, "cdf_lower: %d of %d rows differ from the oracle's, first row %d (range %d..%d, loc %r, scale %r): %s != %s" % (
        bad.size, c["rows"], bad[0], c["row_min"][bad[0]], c["row_max"][bad[0]], c["loc"][bad[0]], c["scale"][bad[0]],
        both_cdf[bad[0]], ref_cdf[bad[0]])
    bad = np.flatnonzero(both_lohi != ref_lohi)
    assert bad.size == 0, "lohi: %d of %d rows differ from the oracle's, first row %d (symbol %r in %d..%d): %#x != %#x" % (
        bad.size, c["rows"], bad[0], c["symbols"][bad[0]], c["row_min"][bad[0]], c["row_max"][bad[0]], both_lohi[bad[0]],
        ref_lohi[bad[0]])
    # the two ways the product calls it: the encoder asks for lohi alone, the decoder for cdf_lower alone
    _, enc_lohi = _laplace_cdf(c, dev_in, False, True)
    dec_cdf, _ = _laplace_cdf(c, dev_in, True, False)
    assert np.array_equal(enc_lohi, ref_lohi), "lohi alone: %d rows differ" % int((enc_lohi != ref_lohi).sum())
    assert np.array_equal(dec_cdf, ref_cdf), "cdf_lower alone: %d rows differ" % int((dec_cdf != ref_cdf).any(1).sum())
    again_cdf, again_lohi = _laplace_cdf(c, dev_in, True, True)             # run-to-run
    assert again_cdf.tobytes() == both_cdf.tobytes() and again_lohi.tobytes() == both_lohi.tobytes()


@pytest.mark.parametrize("ncols", ec.CDF_NCOLS)
def test_laplace_cdf_every_instantiation_both_outputs(ncols):
    """laplace_cdf_kernel<4>, <8>, <16> and <32> at both ends of the ncols interval that selects each: every row of
    cdf_lower is the oracle's sc_get_cdf row (0xFFFF beyond the segment's width), every lohi word is the coded symbol's
    [lower, upper - 1] of that row, whichever outputs are asked for, and twice the same bytes."""
    _check_cdf_launch(ncols)


def test_laplace_cdf_one_row_segments():
    """1000 rows (not a multiple of the block), seg_rows = 1: every row reads a range of its own, widths 2 to 8."""
    _check_cdf_launch(ec.ROWWISE)


# ----------------------------------------------------------------------------
# B. past the caps
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [ec.CAP_LAPLACE + ec.RAGGED, ec.SMALL])
def test_laplace_likelihood_past_the_cap(n):
    """8192 blocks of 256 and 773 elements more, and 257 elements: values and likelihood are oracle.sc_call's bit for bit, with
    rounding and with noise.  The noise path was allowed rtol 2e-5 before it was measured: 0 of 2 097 925 likelihoods differ
    from the oracle's in bits (0 ulp), so it is held to equality like the rounded path and the pmf of the same function."""
    y, loc, scale, noise = ec.laplace_inputs(n)
    yd, ld, sd, nd = (_dev(a) for a in (y, loc, scale, noise))
    for training in (False, True):
        v_ref, lik_ref = ec.laplace_reference(n, training)
        v = torch.full((n,), 9.5, device="cuda")
        lik = torch.full((n,), 9.5, device="cuda")
        _lib.check(_lib.hip().pcgc_laplace_likelihood(_lib.dptr(yd), _lib.dptr(ld), _lib.dptr(sd), _lib.dptr(nd) if training else None,
                                                      _lib.dptr(v), _lib.dptr(lik), n, ec.BOUND, _lib.stream()))
        what = "laplace n=%d %s" % (n, "noise" if training else "rounded")
        _same_bits(v, v_ref, what + " values")
        _ulp_report(lik, lik_ref, what + " likelihood")
        _same_bits(lik, lik_ref, what + " likelihood")
        if not training:
            assert lik_ref[6] == np.float32(ec.BOUND) and lik_ref[n - 1] == np.float32(ec.BOUND)      # the sign(2q - loc) == 0 quirk


@pytest.mark.parametrize("C", ec.FACTORIZED_C)
def test_factorized_likelihood_past_the_cap(C):
    """4096 blocks of 256 and a ragged second sweep (whole rows of C channels: 1 049 352, 1 049 349 and 1 049 408 elements for
    C = 8, 3, 64), and the first multiple of C above 257: values and likelihood are oracle.eb_call's bit for bit, with rounding
    and with noise, and the pmf over [-15, 15] is eb_pmf's.  The likelihood was allowed rtol 5e-5 before it was measured: 0
    elements differ from the oracle's in bits (0 ulp) at every C, size and path, so it is held to equality like the pmf."""
    pd = _dev(ec.factorized_params(C)[1])
    lo, hi = ec.PMF_RANGE
    pmf = torch.full((C, hi - lo + 1), 9.5, device="cuda")
    _lib.check(_lib.hip().pcgc_factorized_pmf(_lib.dptr(pd), C, lo, hi, ec.BOUND, _lib.dptr(pmf), _lib.stream()))
    _same_bits(pmf, ec.factorized_pmf_reference(C), "factorized pmf C=%d" % C)
    for n in (ec.factorized_n(ec.CAP_FACTORIZED + ec.RAGGED, C), ec.factorized_n(ec.SMALL, C)):
        z, noise = ec.factorized_inputs(n, C)
        zd, nd = _dev(z), _dev(noise)
        for training in (False, True):
            v_ref, lik_ref = ec.factorized_reference(n, C, training)
            v = torch.full((n,), 9.5, device="cuda")
            lik = torch.full((n,), 9.5, device="cuda")
            _lib.check(_lib.hip().pcgc_factorized_likelihood(_lib.dptr(zd), _lib.dptr(pd), _lib.dptr(nd) if training else None,
                                                             _lib.dptr(v), _lib.dptr(lik), n, C, ec.BOUND, _lib.stream()))
            what = "factorized C=%d n=%d %s" % (C, n, "noise" if training else "rounded")
            _same_bits(v, v_ref, what + " values")
            _ulp_report(lik, lik_ref, what + " likelihood")
            _same_bits(lik, lik_ref, what + " likelihood")


@pytest.mark.parametrize("n", [ec.CAP_SYMBOLS + ec.RAGGED, ec.SMALL])
def test_symbols_to_values_past_the_cap(n):
    """2048 blocks of 256 and 773 symbols more, and 257 symbols: sym + offset as float32, numpy's bits."""
    sym = ec.symbols(n)[:n]
    out = torch.full((n,), 9.5, device="cuda")
    _lib.check(_lib.hip().pcgc_symbols_to_values(_lib.dptr(_dev(sym)), -15, _lib.dptr(out), n, _lib.stream()))
    _same_bits(out, sym.astype(np.float32) + np.float32(-15), "symbols_to_values n=%d" % n)


def _symbols_seg(sym_d, offs, n, seg_len):
    out = torch.full((n,), 9.5, device="cuda")
    assert out.data_ptr() % 16 == 0
    # one spare entry behind the last segment's: a kernel that looks one offset too far reads a wrong value, not foreign memory
    offs_d = _dev(np.append(offs, np.float32(99.0)))
    _lib.check(_lib.hip().pcgc_symbols_to_values_seg(_lib.dptr(sym_d), _lib.dptr(offs_d), _lib.dptr(out), n, seg_len, _lib.stream()))
    return out


# (segments, seg_len): whole segments only, so "one sweep and a ragged second" is 131 segments of 65 536 = 128 for the sweep of
# the eight-per-thread kernel and three more; then the same data cut into segments of 65 537 and 2 * 65 537 (no multiple of 8)
SEG_LARGE = 131 * 65536


@pytest.mark.parametrize("nseg,seg_len", [(131, 65536), (130, 65537), (65, 2 * 65537), (257, 8), (3, 257)])
def test_symbols_to_values_seg_every_path(nseg, seg_len):
    """out[i] = sym[i] + offset[i // seg_len] by symbols_to_values_seg8_kernel (seg_len a multiple of 8, pointers aligned) and
    by symbols_to_values_seg_kernel (the same symbols read from an odd int16 element, or seg_len no multiple of 8)."""
    n = nseg * seg_len
    big = n > ec.SMALL * 8
    assert n <= SEG_LARGE and (not big or n > ec.CAP_SYMBOLS_SEG8)        # the large cases pass the cap of either kernel
    buf = ec.symbols(SEG_LARGE if big else ec.SMALL * 8)
    buf_d = _dev(buf)
    assert buf_d.data_ptr() % 16 == 0
    offs = ec.seg_offsets(nseg)
    for first in (0, 1):                                       # element 1: sym is 2 bytes off alignment -> the scalar kernel
        sym = buf[first:first + n]
        want = (sym.reshape(nseg, seg_len).astype(np.float32) + offs[:, None]).reshape(-1)
        got = _symbols_seg(buf_d[first:first + n], offs, n, seg_len)
        _same_bits(got, want, "symbols_to_values_seg %d x %d from element %d" % (nseg, seg_len, first))


@pytest.mark.parametrize("fn", range(5))
def test_repro_eval_past_the_cap(fn):
    """exp, log, tanh, sigmoid and softplus of repro_math.h, 4096 blocks of 256 and 773 elements more, and 257 elements: the
    device's bits are the host library's on the same input."""
    for n in (ec.CAP_REPRO + ec.RAGGED, ec.SMALL):
        x = ec.repro_inputs(fn, n)
        want = np.empty_like(x)
        _lib.check_host(_lib.host().pcgc_host_repro_eval(fn, x.ctypes.data_as(ctypes.c_void_p), want.ctypes.data_as(ctypes.c_void_p), n))
        y = torch.full((n,), 9.5, device="cuda")
        _lib.check(_lib.hip().pcgc_repro_eval(fn, _lib.dptr(_dev(x)), _lib.dptr(y), n, _lib.stream()))
        _same_bits(y, want, "repro_eval fn=%d n=%d" % (fn, n))


# ----------------------------------------------------------------------------
# C. pcgc_round_minmax, pcgc_round_minmax_i16
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("seg_len,nseg", ec.MINMAX_CASES)
def test_round_minmax_many_segments(seg_len, nseg):
    """q is numpy's rint bit for bit (the sign of zero included; clamped for int16), every segment's range is numpy's (beyond
    int16 where the values are), with q = NULL too, and twice the same bytes."""
    x = ec.minmax_input(seg_len, nseg)
    q_ref, q16_ref, mn_ref, mx_ref = ec.minmax_reference(seg_len, nseg)
    n = x.size
    xd = _dev(x)
    lib = _lib.hip()

    def run(form):
        q = None if form == "null" else torch.full((n,), 77, dtype=torch.int16 if form == "i16" else torch.float32, device="cuda")
        mm = torch.full((2, nseg), 123456, dtype=torch.int32, device="cuda")
        fn = lib.pcgc_round_minmax_i16 if form == "i16" else lib.pcgc_round_minmax
        _lib.check(fn(_lib.dptr(xd), _lib.dptr(q), _lib.dptr(mm[0]), _lib.dptr(mm[1]), n, seg_len, _lib.stream()))
        return None if q is None else q.cpu().numpy(), mm.cpu().numpy()

    for form, want in (("f32", q_ref), ("i16", q16_ref), ("null", None)):
        q, mm = run(form)
        what = "round_minmax %s %d x %d" % (form, nseg, seg_len)
        if want is not None:
            _same_bits(q, want, what + " q")
        bad = np.flatnonzero((mm[0] != mn_ref) | (mm[1] != mx_ref))
        assert bad.size == 0, "%s: range of %d segments differs, first %d: [%d, %d] != [%d, %d]" % (
            what, bad.size, bad[0], mm[0][bad[0]], mm[1][bad[0]], mn_ref[bad[0]], mx_ref[bad[0]])
        q2, mm2 = run(form)                                                 # run-to-run
        assert mm2.tobytes() == mm.tobytes() and (q is None or q2.tobytes() == q.tobytes())
    assert (mx_ref.max(), mn_ref.min(), q16_ref.max(), q16_ref.min()) == (40000, -40000, 32767, -32768)
