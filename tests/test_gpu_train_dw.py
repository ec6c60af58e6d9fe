"""-m gpu: every weight-gradient kernel of train_dw.hip (and the generic one of train.hip) at a launch where a workgroup walks
several tiles and the workgroups do not all walk equally many (tests/_dw_cases.py; test_dw_cases_host.py proves that coverage
on the CPU), against the float64 reference of tests/_dw_ref.py.  Each case twice:

(a) exact.  x in {0, 1, 2} drawn like a ReLU output, dz in {-1, 0, 1}, stored as float32.  Every product, every partial sum in
    any order and every result is an integer of magnitude at most 2 * 884 736 < 2^24, so float32 arithmetic is exact whatever
    the summation order, and the gradient must EQUAL the reference.  One dropped, doubled or mis-shifted voxel of one tap
    changes an integer: this is the index check.

(b) rounding.  x = relu(randn), dz = randn.  Per element |dk - ref| <= 4 * 2^-24 * sqrt(N * S2), N = voxels summed, S2 = the
    sum of the squared terms: 2^-24 * sqrt(N * S2) is the rms error of a float32 sum of N such terms in the worst (serial)
    order — term k meets a running sum of about sqrt(k * S2 / N), rounded to 2^-24 relative — the kernels sum in hundreds of
    partials and sit far below it, and the factor 4 covers the tail of that error over the 27 * Cin * Cout elements.  The bias
    sums likewise with S2 = sum of dz^2.  This catches operands or sums in reduced precision, which (a) cannot see.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _dw_cases                                              # noqa: E402
from _dw_ref import dw_reference                              # noqa: E402

U24 = 2.0 ** -24


def _shapes(case):
    """(ksize, cin, cout, stride, transposed, D, B, Dout, filter shape)"""
    if case[0] == "pair":
        _, cin, cout, D, B = case
        return 3, cin, cout, 1, 0, D, B, D, (3, 3, 3, cin, cout)
    k, cin, cout, stride, tr, D, B = case
    Dout = 2 * D if tr else D // stride
    return k, cin, cout, stride, tr, D, B, Dout, ((k, k, k, cout, cin) if tr else (k, k, k, cin, cout))


def _operands(case, kind, dev, n_dz=1):
    """x and n_dz output gradients, seeded per case: small integers (kind 'int') or Gaussians, as float32 on the device."""
    k, cin, cout, stride, tr, D, B, Dout, _ = _shapes(case)
    g = torch.Generator(device=dev).manual_seed(1000 * _dw_cases.CASES.index(case) + (7 if kind == "int" else 11))
    xs, zs = (B, D, D, D, cin), (B, Dout, Dout, Dout, cout)
    if kind == "int":
        x = torch.randint(-2, 3, xs, generator=g, device=dev).clamp_(min=0).float()          # 0 three times in five, like a ReLU
        dzs = [torch.randint(-1, 2, zs, generator=g, device=dev).float() for _ in range(n_dz)]
    else:
        x = torch.relu(torch.randn(xs, generator=g, device=dev))
        dzs = [torch.randn(zs, generator=g, device=dev) for _ in range(n_dz)]
    return x, dzs


def _sentinel(shape, dev):
    return torch.full(shape, float("nan"), device=dev)       # an element the call does not write stays NaN and equals nothing


def _single(case, x, dz, dev):
    """pcgc_conv3d_bwd_weight -> (dkernel, dbias)"""
    from pcgcv1_amd import _lib
    lib = _lib.hip()
    k, cin, cout, stride, tr, D, B, Dout, kshape = _shapes(case)
    n = int(lib.pcgc_conv3d_bwd_workspace_bytes(cin, cout, k))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    gk, gb = _sentinel(kshape, dev), _sentinel((cout,), dev)
    _lib.check(lib.pcgc_conv3d_bwd_weight(_lib.dptr(x), _lib.dptr(dz), _lib.dptr(gk), _lib.dptr(gb), B, D, cin, cout, k, stride, tr,
                                          _lib.dptr(ws), n, _lib.stream()), "pcgc_conv3d_bwd_weight")
    torch.cuda.synchronize()
    return gk, gb


def _pair(case, x, dz3, dz1, dev):
    """One training plan, layers 0 (3^3) and 1 (1^3) through pcgc_train_conv_bwd_weight_pair, layer 2 (3^3) through the single
    call on the same operands -> [(dkernel, dbias)] * 3"""
    from pcgcv1_amd import _lib
    from pcgcv1_amd.train_hyper import _TrainLayer
    lib = _lib.hip()
    _, cin, cout, _, _, D, B, _, _ = _shapes(case)
    shapes = [(cin, cout, 3), (cin, cout, 1), (cin, cout, 3)]
    ks = [torch.zeros((k, k, k, ci, co), device=dev) for ci, co, k in shapes]
    out = [(_sentinel(k_.shape, dev), _sentinel((cout,), dev)) for k_ in ks]
    arr = (_TrainLayer * len(shapes))()
    for i, (ci, co, k) in enumerate(shapes):
        arr[i].kernel, arr[i].dkernel, arr[i].dbias = ks[i].data_ptr(), out[i][0].data_ptr(), out[i][1].data_ptr()
        arr[i].Cin, arr[i].Cout, arr[i].ksize, arr[i].stride, arr[i].transposed = ci, co, k, 1, 0
    plan = ctypes.c_void_p()
    _lib.check(lib.pcgc_train_plan_create(ctypes.cast(arr, ctypes.c_void_p), len(shapes), ctypes.byref(plan)), "pcgc_train_plan_create")
    try:
        st = _lib.stream()
        _lib.check(lib.pcgc_train_plan_prepare(plan, st), "pcgc_train_plan_prepare")
        _lib.check(lib.pcgc_train_conv_bwd_weight_pair(plan, 0, 1, _lib.dptr(x), _lib.dptr(dz3), _lib.dptr(dz1), B, D, st), "bwd_weight_pair")
        _lib.check(lib.pcgc_train_conv_bwd_weight(plan, 2, _lib.dptr(x), _lib.dptr(dz3), B, D, st), "bwd_weight")
        _lib.check(lib.pcgc_train_plan_finish_weights(plan, st), "pcgc_train_plan_finish_weights")
        torch.cuda.synchronize()
    finally:
        lib.pcgc_train_plan_destroy(plan)
    return out


def _run(case, kind, dev):
    """-> [(what, dkernel, dbias, reference)] for the layers of the case, and the extra single-call result of a pair"""
    k, cin, cout, stride, tr, *_ = _shapes(case)
    if case[0] == "pair":
        x, (dz3, dz1) = _operands(case, kind, dev, n_dz=2)
        (gk3, gb3), (gk1, gb1), single = _pair(case, x, dz3, dz1, dev)
        return [("3^3 of the pair", gk3, gb3, dw_reference(x, dz3, 3)), ("1^3 of the pair", gk1, gb1, dw_reference(x, dz1, 1))], single, \
            lambda: _pair(case, x, dz3, dz1, dev)[:2]
    x, (dz,) = _operands(case, kind, dev)
    gk, gb = _single(case, x, dz, dev)
    return [("layer", gk, gb, dw_reference(x, dz, k, stride, bool(tr)))], None, lambda: [_single(case, x, dz, dev)]


@pytest.mark.parametrize("case", _dw_cases.CASES, ids=_dw_cases.case_id)
def test_weight_gradient_at_a_multi_tile_uneven_launch(case):
    from pcgcv1_amd import _lib
    dev = _lib.require_gpu()

    # (a) integers: equality
    layers, single, _ = _run(case, "int", dev)
    for what, gk, gb, ref in layers:
        assert float(ref.dk.abs().max()) > 0 and 2 * max(ref.n, ref.nb) < 2 ** 24, what       # |x dz| <= 2: sums of N terms stay exact
        np.testing.assert_array_equal(gk.double().cpu().numpy(), ref.dk.cpu().numpy(), err_msg="%s %s: filter gradient" % (case, what))
        np.testing.assert_array_equal(gb.double().cpu().numpy(), ref.db.cpu().numpy(), err_msg="%s %s: bias sums" % (case, what))
    if single is not None:                                    # the 3^3 half of the pair kernel = the single call, bit for bit
        assert torch.equal(layers[0][1], single[0]) and torch.equal(layers[0][2], single[1])

    # (b) Gaussians: inside the float32 summation bound, element by element
    layers, single, again = _run(case, "gauss", dev)
    for what, gk, gb, ref in layers:
        bound_k = 4.0 * U24 * torch.sqrt(ref.n * ref.s2k)
        bound_b = 4.0 * U24 * torch.sqrt(ref.nb * ref.s2b)
        assert float(bound_k.min()) > 0 and float(bound_b.min()) > 0
        assert torch.isfinite(gk).all() and torch.isfinite(gb).all(), what
        rk =float(((gk.double() - ref.dk).abs() / bound_k).max())
        rb = float(((gb.double() - ref.db).abs() / bound_b).max())
        print("%s %s: worst err / bound  filter %.4f  bias %.4f  (N = %d)" % (_dw_cases.case_id(case), what, rk, rb, ref.n))
        assert rk <= 1.0, "%s %s: filter gradient %.3f of the bound" % (case, what, rk)
        assert rb <= 1.0, "%s %s: bias sums %.3f of the bound" % (case, what, rb)
    if single is not None:
        assert torch.equal(layers[0][1], single[0]) and torch.equal(layers[0][2], single[1])
    # fixed summation order: the same operands give the same bits
    for (what, gk, gb, _), (gk2, gb2) in zip(layers, again()):
        assert torch.equal(gk, gk2) and torch.equal(gb, gb2), what
