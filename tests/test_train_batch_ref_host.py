"""CPU: the float64 references of tests/_train_batch_ref.py against the oracle, and the condition under which the integer rows of
tests/test_gpu_train_batch.py may demand EQUALITY.

1. block_reference == oracle.nets (torch's float32 convolutions, layer by layer and as vrn_block) on integer operands, where both
   are exact, and within float32 rounding of it on Gaussian operands; sign_words against a bit loop.
2. conv_adjoint == float64 autograd of oracle/train.py:_conv for every layer shape of the table (smaller cubes), and the
   mask / add_to formula around it.
3. Exactness: for every case of the table, the sum of |terms| of every output is below 2^24 — derived from the operands' RANGES
   and the shapes (block_abs_bound, adjoint_abs_bound), not measured; the ranges are those the generators produce (asserted on
   drawn operands), and on a drawn block the true sums of |terms| stay under the derived ones.
4. The integer block is not degenerate: between 5 % and 95 % of `pre` is positive, every kept tensor has non-zero entries.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import nets as onets                          # noqa: E402
from oracle import train as otrain                        # noqa: E402
import _train_batch_ref as R                              # noqa: E402


def _w_dict(params):
    names = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv2_3")
    w = {}
    for i, n in enumerate(names):
        w["b/%s/kernel" % n], w["b/%s/bias" % n] = params[2 * i].numpy(), params[2 * i + 1].numpy()
    return w


def _oracle_block(x, params):
    w, xn = _w_dict(params), x.numpy()
    t11 = onets._conv(w, "b/conv1_1", xn, relu=True)
    t12 = onets._conv(w, "b/conv1_2", t11, relu=True)
    t21 = onets._conv(w, "b/conv2_1", xn, relu=True)
    t22 = onets._conv(w, "b/conv2_2", t21, relu=True)
    t23 = onets._conv(w, "b/conv2_3", t22, relu=True)
    return R.Block(t11, t21, t22, np.concatenate([t12, t23], -1), onets.vrn_block(w, "b", xn))


def test_block_reference_equals_the_oracle_on_integers_and_tracks_it_on_gaussians():
    x, params = R.block_operands("int", 2, 8, 32, seed=3)
    ref, ora = R.block_reference(x, params), _oracle_block(x, params)
    for name in R.Block._fields:
        got, want = getattr(ref, name).numpy(), getattr(ora, name).astype(np.float64)
        assert np.abs(want).max() > 0, name
        np.testing.assert_array_equal(got, want, err_msg=name)
    x, params = R.block_operands("gauss", 2, 8, 32, seed=4)
    ref, ora = R.block_reference(x, params), _oracle_block(x, params)
    for name in R.Block._fields:
        got, want = getattr(ref, name).numpy(), getattr(ora, name).astype(np.float64)
        assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), name      # the oracle here is float32
    # the faces are those of test_vrn_block_vs_oracle
    assert float(x[0, 0, 3, 3, 0]) == 1.5 and float(x[0, 3, 3, -1, 0]) == 3.0 and float(x[0, -1, 3, 3, 5]) == -0.5


def test_sign_words_are_the_bits_of_pre():
    g = torch.Generator().manual_seed(1)
    pre = torch.randn((2, 3, 3, 3, 32), generator=g, dtype=torch.float64)
    pre[0, 0, 0, 0] = 1.0                                      # all 32 bits set: the word is -1
    pre[0, 0, 0, 1] = -1.0
    words = R.sign_words(pre)
    assert words.dtype == torch.int32 and int(words[0, 0, 0, 0]) == -1 and int(words[0, 0, 0, 1]) == 0
    for c in range(32):
        assert torch.equal(((words >> c) & 1).bool(), pre[..., c] > 0), c


@pytest.mark.parametrize("layer", R.BWD_LAYERS, ids=lambda l: "%dto%d-k%d-s%d-t%d" % l[:5])
def test_conv_adjoint_equals_float64_autograd_of_the_oracle_convolution(layer):
    cin, cout, k, stride, tr, _ = layer
    D, B = (8 if stride == 2 and not tr else 4), 2            # the smallest cubes with an interior voxel and every border
    ops = R.bwd_data_operands("gauss", (cin, cout, k, stride, tr, D), B, seed=cin + 7 * cout + k)
    nc = lambda t: t.permute(0, 4, 1, 2, 3).contiguous()
    xt = torch.zeros(R.layer_shapes(cin, cout, k, stride, tr, D, B)[2], dtype=torch.float64)
    xt = nc(xt).requires_grad_(True)
    y = otrain._conv({"l/kernel": ops["w"].double()}, "l", xt, stride=stride, tconv=bool(tr))
    (adj,) = torch.autograd.grad(y, xt, nc(ops["dz"].double()))
    adj = adj.permute(0, 2, 3, 4, 1)
    got = R.conv_adjoint(ops["dz"].double(), ops["w"].double(), D, stride, bool(tr))
    assert float(adj.abs().max()) > 0
    assert float((got - adj).abs().max()) <= 1e-12 * float(adj.abs().max())
    full = R.bwd_data_reference(ops["dz"], ops["w"], D, stride, bool(tr), mask=ops["mask"], add_to=ops["add_to"])
    want = (adj + ops["add_to"].double()) * (ops["mask"] > 0).double()
    assert float((full - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert 0.2 < float((ops["mask"] > 0).float().mean()) < 0.8


def test_integer_rows_are_exact_in_float32_whatever_the_summation_order():
    # the ranges the generators produce
    for B, D, C in R.BLOCK_CASES:
        x, params = R.block_operands("int", 1, 8, C, seed=B)
        assert float(x.min()) == 0 and float(x.max()) == R.X_MAX and torch.equal(x, x.round())
        for p in params:
            top = R.BIAS_MAX if p.dim() == 1 else R.W_MAX
            assert float(p.abs().max()) <= top and torch.equal(p, p.round())
        # from the ranges: the block's largest sums of |terms|
        bound = R.block_abs_bound(C)
        assert bound["t11"] == 27 * 32 * 2 + 2 and bound["t12"] == 27 * 8 * (27 * 32 * 2 + 2) + 2 == 373682      # the conv1_2 path
        assert bound["t23"] == 8 * (27 * 8 * (32 * 2 + 2) + 2) + 2 == 114066                                      # the conv2_3 path
        assert max(bound.values()) < R.EXACT
        # ... and a drawn block stays under them: sums of |terms| = the same convolutions on |x|, |w|, |b|
        ab = [p.abs().double() for p in params]
        a11 = R.conv_same(x.double(), ab[0], ab[1])
        a12 = R.conv_same(a11, ab[2], ab[3])
        a21 = R.conv_same(x.double(), ab[4], ab[5])
        a22 = R.conv_same(a21, ab[6], ab[7])
        a23 = R.conv_same(a22, ab[8], ab[9])
        for name, a in (("t11", a11), ("t12", a12), ("t21", a21), ("t22", a22), ("t23", a23)):
            assert 0 < float(a.max()) <= bound[name], name
    for layer, B in R.BWD_CASES:
        cin, cout, k, stride, tr, D = layer
        ops = R.bwd_data_operands("int", (cin, cout, k, stride, tr, 8 if stride == 2 and not tr else 4), 1, seed=B)
        for name, top in (("dz", R.DZ_MAX), ("w", R.W_MAX), ("add_to", R.ADD_MAX), ("mask", R.X_MAX)):
            assert 0 < float(ops[name].abs().max()) <= top and torch.equal(ops[name], ops[name].round()), name
        bound = R.adjoint_abs_bound(cout, k)
        assert bound <= 27 * 64 * 2 + R.ADD_MAX and bound < R.EXACT
        got = R.conv_adjoint(ops["dz"].abs().double(), ops["w"].abs().double(), ops["mask"].shape[1], stride, bool(tr)) + ops["add_to"].abs().double()
        assert 0 < float(got.max()) <= bound


def test_the_table_stands_on_both_sides_of_each_threshold():
    assert [B for B, _, _ in R.BLOCK_CASES] == [16, 17]
    for layer in R.BWD_LAYERS:
        assert R.is_small_launch(layer, 19) and not R.is_small_launch(layer, 20), layer
        assert (layer, 19) in R.BWD_CASES and (layer, 20) in R.BWD_CASES
    wide = (64, 16, 3, 1, 0, 32)
    assert R.is_small_launch(wide, 2) and not R.is_small_launch(wide, 3) and (wide, 2) in R.BWD_CASES and (wide, 3) in R.BWD_CASES
    assert R.is_small_launch(R.BWD_LAYERS[0], 1) and R.is_small_launch(wide, 1)          # the single-cube launches: the other form


def test_integer_block_is_not_degenerate():
    x, params = R.block_operands("int", 2, 8, 32, seed=17)
    ref = R.block_reference(x, params)
    frac = float((ref.pre > 0).double().mean())
    assert 0.05 < frac < 0.95, frac
    for half in (ref.pre[..., :16], ref.pre[..., 16:]):
        assert 0.05 < float((half > 0).double().mean()) < 0.95
    for name in R.Block._fields:
        t = getattr(ref, name)
        assert float(t.max()) > 0 and float((t == 0).double().mean()) > 0.01, name
    assert not torch.equal(x[0], x[1])
