"""-m gpu: the train_hyper step against the CPU oracle (oracle/train.py, torch autograd)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import train as otrain                      # noqa: E402
from pcgcv1_amd import synthetic                          # noqa: E402
from pcgcv1_amd.train_hyper import Trainer                # noqa: E402


def _setup(seed=5, B=2, cs=16):
    w = synthetic.make_weights(seed=seed, profile="dense")
    # move the likelihoods away from their 1e-9 floor so that every gradient path is exercised
    w["hyper_decoder/conv4_2/bias"] = (w["hyper_decoder/conv4_2/bias"] + 0.8).astype(np.float32)
    x = synthetic.make_cubes(seed=seed, n_cubes=B, cube_size=cs, occupancy=0.06)
    rng = np.random.default_rng(seed)
    ny = (rng.random((B, cs // 4, cs // 4, cs // 4, 16)) - 0.5).astype(np.float32)
    nz = (rng.random((B, cs // 8, cs // 8, cs // 8, 8)) - 0.5).astype(np.float32)
    return w, x, ny, nz


def test_loss_terms_and_gradients_match_autograd():
    w, x, ny, nz = _setup()
    alpha, beta = 0.75, 3.0
    terms_ref, leaves = otrain.forward_loss(w, x, ny, nz, alpha, beta)
    tr = Trainer(w, alpha=alpha, beta=beta)
    terms = tr.forward_backward(x, ny, nz)
    for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
        assert abs(terms[k] - terms_ref[k]) <= 2e-4 * max(1.0, abs(terms_ref[k])), (k, terms[k], terms_ref[k])
    worst = []
    for name, leaf in leaves.items():
        g_ref = leaf.grad.numpy()
        g = tr.g[name].cpu().numpy()
        scale = float(np.abs(g_ref).max())
        assert scale > 0, name + ": oracle gradient is identically zero (test does not exercise it)"
        err = float(np.abs(g - g_ref).max()) / scale
        worst.append((err, name))
        assert err < 5e-3, (name, err, scale)
    print(sorted(worst)[-3:])


def test_full_size_gradients_match_autograd_at_64():
    """The same comparison at the size the step really runs at: one 64^3 cube through every fused path of the training
    step (row-kernel forward of the 64^3 / 32^3 blocks, the one-pass block reverses, sliding-kw / matrix-core weight
    gradients, the 8^3 hyper row kernels) — loss terms and ALL parameter gradients against torch autograd on the CPU
    (oracle/train.py).  At 16^3 none of the 64^3-only kernels is taken."""
    w, x, ny, nz = _setup(seed=12, B=1, cs=64)
    alpha, beta = 0.75, 3.0
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    terms_ref, leaves = otrain.forward_loss(w, x, ny, nz, alpha, beta)
    tr = Trainer(w, alpha=alpha, beta=beta)
    terms = tr.forward_backward(x, ny, nz)
    for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
        assert abs(terms[k] - terms_ref[k]) <= 2e-4 * max(1.0, abs(terms_ref[k])), (k, terms[k], terms_ref[k])
    worst = []
    for name, leaf in leaves.items():
        g_ref = leaf.grad.numpy()
        g = tr.g[name].cpu().numpy()
        scale = float(np.abs(g_ref).max())
        assert scale > 0, name
        err = float(np.abs(g - g_ref).max()) / scale
        worst.append((err, name))
        assert err < 5e-3, (name, err, scale)
    print(sorted(worst)[-3:])


def test_q4_training_layout_gives_the_same_step():
    """Trainer(q4=True) — the default: the 64^3 stage's 16-channel tensors and the blocks' 8-channel gradients in the Q4
    layout of the inference path — against Trainer(q4=False) (everything NDHWC) on two cubes of 64^3 with the same weights
    and noise: same loss terms and the same gradient for every parameter.  The blocks' row kernels and every weight-
    gradient kernel form the same sums from other addresses; conv_in / deconv_out run on the inference path's row kernels
    in Q4 mode (another summation order), hence a tolerance and not bit-equality.  The autograd comparison above runs in Q4
    mode; this one pins the two layouts to each other at a batch of more than one cube."""
    # seed: one without a bit-exact y~ -+ 0.5 == loc in either step.  At such a tie the gradient of tf.abs is 0 and the Laplace
    # reverse kernel drops that edge's density; the two steps' y differ in the last place, so a tie in one of them alone (seed
    # 13: one element of the Q4 step) parts them by one element's worth, like the ReLU flips below (2.09e-4 on one tensor)
    w, x, ny, nz = _setup(seed=17, B=2, cs=64)
    a = Trainer(w, alpha=0.75, beta=3.0, q4=True)
    b = Trainer(w, alpha=0.75, beta=3.0, q4=False)
    tb = b.forward_backward(x, ny, nz)
    # (1) layout against layout with the same kernels everywhere else: up_2 / down_1 of the Q4 step on the implicit-GEMM kernels
    #     the NDHWC step uses (PCGC_TRAIN_ROW_RESAMPLE=0);  (2) the shipped Q4 step, whose up_2 / down_1 (forward and reverse)
    #     run on the inference path's row kernels since round 5 — four more layers that sum in another order, and a ReLU that
    #     flips on a value within 1e-7 of zero moves a weight gradient by one voxel's worth: a wider bound, still an order
    #     of magnitude inside the 5e-3 the autograd comparison above allows
    for env, tol in (("0", 2e-4), ("1", 6e-4)):
        os.environ["PCGC_TRAIN_ROW_RESAMPLE"] = env
        try:
            ta = a.forward_backward(x, ny, nz)
        finally:
            os.environ.pop("PCGC_TRAIN_ROW_RESAMPLE", None)
        assert a._q4_active is True and b._q4_active is False
        for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
            assert abs(ta[k] - tb[k]) <= 1e-5 * max(1.0, abs(tb[k])), (k, ta[k], tb[k])
        worst = []
        for name in a.g:
            ga, gb = a.g[name].cpu().numpy(), b.g[name].cpu().numpy()
            scale = float(np.abs(gb).max())
            assert scale > 0, name
            err = float(np.abs(ga - gb).max()) / scale
            worst.append((err, name))
            assert err < tol, (env, name, err, scale)
        print("PCGC_TRAIN_ROW_RESAMPLE=%s:" % env, sorted(worst)[-3:])
    # the layout follows the cube size: at 16^3 nothing is Q4 (no kernel of the stage exists there) and the step still runs
    w16, x16, ny16, nz16 = _setup(seed=6)
    a.forward_backward(x16, ny16, nz16)
    assert a._q4_active is False


def test_deferred_small_weight_gradients_are_bit_identical(monkeypatch):
    """pcgc_train_plan_defer_small (the Trainer's default): the 16^3 stage's weight gradients launched at the end of the reverse
    pass, equal shapes as the jobs of one launch, against every layer's own launch (PCGC_TRAIN_DEFER_DW=0) — same kernels, same
    tiles, same partial buffers: every gradient bit for bit, with garbage written over freed memory in between (a deferred job
    whose operand had been released would read it)."""
    w, x, ny, nz = _setup(seed=17, B=2, cs=64)
    monkeypatch.setenv("PCGC_TRAIN_DEFER_DW", "0")
    a = Trainer(w, alpha=0.75, beta=3.0)
    monkeypatch.setenv("PCGC_TRAIN_DEFER_DW", "1")
    b = Trainer(w, alpha=0.75, beta=3.0)
    assert a._defer is False and b._defer is True
    ta = a.forward_backward(x, ny, nz)
    tb = b.forward_backward(x, ny, nz)
    assert not b._held
    for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
        assert ta[k] == tb[k], k
    assert torch.equal(a.flat_g, b.flat_g)
    assert float(a.flat_g.abs().max()) > 0
    # twice in a row (the pool is right-sized now), and the small-cube step (stride-1 layers at D = 16, 8 and 4)
    tb2 = b.forward_backward(x, ny, nz)
    assert torch.equal(a.flat_g, b.flat_g) and tb2["loss"] == tb["loss"]
    w16, x16, ny16, nz16 = _setup(seed=6)
    a.forward_backward(x16, ny16, nz16)
    b.forward_backward(x16, ny16, nz16)
    assert torch.equal(a.flat_g, b.flat_g)


def test_pair_launches_of_the_16_cubed_blocks_are_bit_identical(monkeypatch):
    """pcgc_train_conv_fwd_pair / pcgc_train_conv_bwd_data_pair (two independent stride-1 layers of a 16^3 block in one launch:
    conv1_1 | conv2_1, conv1_2 | conv2_2, conv1_2^T | conv2_3^T), pcgc_train_conv_fwd_merge (conv2_3, then the block's merge on the
    same tiles) and pcgc_train_conv_bwd_data_chain (conv1_1^T, then conv2_1^T adding to the same tiles) against the layers one by
    one (PCGC_CONV_PAIRS=0, read per call): the same tiles and sums, so every loss term and every gradient bit for bit — on a 64^3 batch (its 16^3 stage) and
    on 16^3 cubes (pairs at D = 16; the D = 4 stage and shapes without a pair kernel take the single calls inside)."""
    for seed, B, cs in ((17, 2, 64), (6, 2, 16), (9, 8, 16)):
        w, x, ny, nz = _setup(seed=seed, B=B, cs=cs)
        tr = Trainer(w, alpha=0.75, beta=3.0)
        monkeypatch.setenv("PCGC_CONV_PAIRS", "0")
        monkeypatch.setenv("PCGC_CONV_PIPE", "0")
        ta = tr.forward_backward(x, ny, nz)
        ga = tr.flat_g.clone()
        # ... and the software-pipelined form of the small launches (conv_mfma_small_body, tconv_mfma_small_kernel: the same
        # MFMAs in the same order with the loads moved ahead) against conv_mfma_body / tconv_mfma_kernel (PCGC_CONV_PIPE=0)
        for pairs, pipe in (("1", "0"), ("0", "1"), ("1", "1")):
            monkeypatch.setenv("PCGC_CONV_PAIRS", pairs)
            monkeypatch.setenv("PCGC_CONV_PIPE", pipe)
            tb = tr.forward_backward(x, ny, nz)
            for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
                assert ta[k] == tb[k], (k, cs, pairs, pipe)
            assert torch.equal(ga, tr.flat_g) and float(ga.abs().max()) > 0, (cs, pairs, pipe)


def test_step_on_a_batch_without_occupied_voxels_raises_and_leaves_the_model_alone():
    """Trainer.step queues the optimiser update BEFORE it reads the loss terms back (pcgc_adam_step_guarded); a batch whose BCE
    averages divide by zero (loss.py:8-33) must still raise, with parameters, Adam slots and the step count untouched — the
    update is skipped on the device — and the next good step must be the step a fresh trainer takes."""
    w, x, ny, nz = _setup(seed=21, B=2, cs=16)
    a, b = Trainer(w, alpha=0.75, beta=3.0, lr=1e-3), Trainer(w, alpha=0.75, beta=3.0, lr=1e-3)
    p0, m0, v0 = a.flat_p.clone(), a.flat_m.clone(), a.flat_v.clone()
    with pytest.raises(ZeroDivisionError):
        a.step(np.zeros_like(x), ny, nz)
    assert a.t == 0 and torch.equal(a.flat_p, p0) and torch.equal(a.flat_m, m0) and torch.equal(a.flat_v, v0)
    assert float(a.flat_g.abs().max()) == 0.0
    ta, tb = a.step(x, ny, nz), b.step(x, ny, nz)
    assert a.t == b.t == 1 and ta["loss"] == tb["loss"]
    assert torch.equal(a.flat_p, b.flat_p) and not torch.equal(a.flat_p, p0)


def test_weight_gradients_on_their_own_stream_are_bit_identical(monkeypatch):
    """The Trainer's default sends the 64^3 / 32^3 stages' weight-gradient launches to a second stream (next to the chain of
    bwd-data kernels) and joins it before the final sums; against PCGC_TRAIN_DW_STREAM=0 (one stream): every loss term and
    gradient bit for bit, three steps in a row, with PCGC_DEBUG_HELD-style checksums of the held operands taken on the way
    (an operand written on the main stream before the side stream read it would change a gradient — and the checksum)."""
    from pcgcv1_amd import train_hyper
    w, x, ny, nz = _setup(seed=23, B=2, cs=64)
    monkeypatch.setenv("PCGC_TRAIN_DW_STREAM", "0")
    a = Trainer(w, alpha=0.75, beta=3.0, lr=1e-4)
    monkeypatch.setenv("PCGC_TRAIN_DW_STREAM", "1")
    b = Trainer(w, alpha=0.75, beta=3.0, lr=1e-4)
    assert a._dw_stream is None and b._dw_stream is not None
    monkeypatch.setattr(train_hyper, "_DEBUG_HELD", True)
    for _ in range(3):
        ta, tb = a.step(x, ny, nz), b.step(x, ny, nz)
        for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
            assert ta[k] == tb[k], k
        assert torch.equal(a.flat_g, b.flat_g) and torch.equal(a.flat_p, b.flat_p)
    assert float(a.flat_g.abs().max()) > 0 and not b._held


def test_fused_loss_sums_equal_the_separate_reductions():
    """pcgc_train_loss_sums (the step's BCE sums and both log-likelihood sums in two launches) == pcgc_bce_sums + 2 x
    pcgc_sum_log, bit for bit (the same blocks run the same fixed-order sums)."""
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(77)
    for n, ny, nz in ((2 * 64 ** 3, 2 * 16 ** 3 * 16, 2 * 8 ** 3 * 8), (1000, 77, 5)):
        pred = (torch.randn(n, generator=g) * 3).to(dev)
        label = (torch.rand(n, generator=g) < 0.05).float().to(dev)
        lik_y = (torch.rand(ny, generator=g) * 0.9 + 1e-6).to(dev)
        lik_z = (torch.rand(nz, generator=g) * 0.9 + 1e-6).to(dev)
        a4, a2 = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.pcgc_bce_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        ws2 = torch.empty(int(lib.pcgc_sum_log_workspace_bytes()), dtype=torch.uint8, device=dev)
        _lib.check(lib.pcgc_bce_sums(_lib.dptr(pred), _lib.dptr(label), n, _lib.dptr(a4), _lib.dptr(ws), ws.numel(), _lib.stream()))
        _lib.check(lib.pcgc_sum_log(_lib.dptr(lik_y), ny, _lib.dptr(a2[0:1]), _lib.dptr(ws2), ws2.numel(), _lib.stream()))
        _lib.check(lib.pcgc_sum_log(_lib.dptr(lik_z), nz, _lib.dptr(a2[1:2]), _lib.dptr(ws2), ws2.numel(), _lib.stream()))
        b = torch.empty(6, dtype=torch.float64, device=dev)
        ws3 = torch.empty(int(lib.pcgc_train_loss_sums_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        _lib.check(lib.pcgc_train_loss_sums(_lib.dptr(pred), _lib.dptr(label), n, _lib.dptr(lik_y), ny, _lib.dptr(lik_z), nz,
                                            _lib.dptr(b[:4]), _lib.dptr(b[4:]), _lib.dptr(ws3), ws3.numel(), _lib.stream()))
        assert torch.equal(b[:4], a4) and torch.equal(b[4:], a2), (n, b, a4, a2)
        assert float(a4[1] + a4[3]) == n


def test_adam_step_matches_tf1_form():
    w, x, ny, nz = _setup(seed=6)
    tr = Trainer(w, alpha=2.0, beta=3.0, lr=1e-3)
    tr.forward_backward(x, ny, nz)
    g = {k: v.cpu().numpy().copy() for k, v in tr.g.items()}
    tr.apply_gradients()
    tr.forward_backward(x, ny, nz)
    g2 = {k: v.cpu().numpy().copy() for k, v in tr.g.items()}
    tr.apply_gradients()
    new = tr.weights()
    for name in ("analysis_transform/conv_in/kernel", "hyper_decoder/conv4_2/bias", "estimator/matrix_1"):
        p, m, v = np.asarray(w[name], np.float32), 0.0, 0.0
        p, m, v = otrain.adam_step(p, g[name], m, v, 1, lr=1e-3)
        p, m, v = otrain.adam_step(p, g2[name], m, v, 2, lr=1e-3)
        np.testing.assert_allclose(new[name], p, rtol=2e-5, atol=1e-7)


def test_training_reduces_the_loss():
    w, x, ny, nz = _setup(seed=7)
    tr = Trainer(w, alpha=0.75, beta=3.0, lr=2e-4)
    first = tr.step(x, ny, nz)["loss"]
    for _ in range(5):
        terms = tr.step(x, ny, nz, with_iou=True)
        last = terms["loss"]
    assert np.isfinite(last) and last < first, (first, last)
    assert 0.0 <= terms["IoU"] <= 1.0                         # top-k classification + get_classify_metrics (train_hyper.py:216-226)


def test_config4_full_size_step():
    """BASELINE configs[3] at its per-GPU shape: batch 8 cubes of 64^3 (train_hyper.py:174-214).  The oracle cannot
    run this size in seconds, so the properties checked are size-independent: two trainers fed the same batch and
    noise produce bit-identical gradients and weights (fixed-order sums in every tile / dW kernel at D = 64), the loss is
    finite and decreases over a few steps, every gradient is finite and non-zero, and the step's device memory stays
    bounded (the unfused layer graph keeps every activation: about 4.6 GiB at this size)."""
    w, _, _, _ = _setup(seed=8)
    x = synthetic.make_cubes(seed=8, n_cubes=8, cube_size=64)
    rng = np.random.default_rng(8)
    ny = (rng.random((8, 16, 16, 16, 16)) - 0.5).astype(np.float32)
    nz = (rng.random((8, 8, 8, 8, 8)) - 0.5).astype(np.float32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = Trainer(w, alpha=0.75, beta=3.0, lr=1e-4), Trainer(w, alpha=0.75, beta=3.0, lr=1e-4)
    ta = a.forward_backward(x, ny, nz)
    tb = b.forward_backward(x, ny, nz)
    assert ta == tb
    assert torch.equal(a.flat_g, b.flat_g)
    g = a.flat_g.cpu().numpy()
    assert np.isfinite(g).all()
    for name, view in a.g.items():
        assert float(view.abs().max()) > 0, name
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 6 * 2 ** 30, "train step peak device memory %.2f GiB" % (peak / 2 ** 30)
    losses = [a.step(x, ny, nz)["loss"] for _ in range(4)]
    for _ in range(4):
        b.step(x, ny, nz)
    assert torch.equal(a.flat_p, b.flat_p)                       # 4 optimiser steps later still the same bits
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0] < ta["loss"] + 1e-9, (ta["loss"], losses)


_BWD_CASES = [  # (Cin, Cout, k, stride, transposed, D of the layer input): every forward shape the nets use
    (16, 4, 3, 1, 0, 16), (4, 8, 3, 1, 0, 16), (4, 4, 3, 1, 0, 16), (16, 4, 1, 1, 0, 16), (4, 8, 1, 1, 0, 16),
    (32, 8, 3, 1, 0, 16), (8, 16, 3, 1, 0, 16), (8, 8, 3, 1, 0, 16), (32, 8, 1, 1, 0, 16), (8, 16, 1, 1, 0, 16),
    (64, 16, 3, 1, 0, 16), (16, 32, 3, 1, 0, 16), (16, 16, 3, 1, 0, 16), (64, 16, 1, 1, 0, 16), (16, 32, 1, 1, 0, 16),
    (16, 64, 3, 1, 0, 16), (16, 1, 3, 1, 0, 16), (1, 16, 3, 1, 0, 16), (32, 16, 3, 1, 0, 16),
    (16, 32, 3, 2, 0, 32), (32, 64, 3, 2, 0, 32), (16, 16, 3, 2, 0, 32),
    (64, 32, 3, 2, 1, 16), (32, 16, 3, 2, 1, 16), (16, 16, 3, 2, 1, 16),
    (16, 4, 3, 1, 0, 8), (16, 32, 3, 2, 0, 8), (32, 16, 3, 2, 1, 4),      # small cubes: generic kernel
    (1, 32, 9, 2, 0, 16), (32, 32, 5, 2, 0, 8), (32, 32, 5, 2, 1, 4), (32, 1, 9, 2, 1, 8),      # model_simple.py shapes
    # shapes of no net at a D the tiled kernels take: the generic kernel (csrc/dw_plan.h has no row for them)
    (8, 32, 3, 1, 0, 16), (8, 4, 3, 1, 0, 16), (4, 16, 3, 1, 0, 16), (32, 1, 3, 1, 0, 16), (32, 4, 1, 1, 0, 16),
]


@pytest.mark.parametrize("cin,cout,k,stride,tr,D", _BWD_CASES)
def test_conv_bwd_data_and_weight_match_autograd(cin, cout, k, stride, tr, D):
    """pcgc_conv3d_bwd_data / _bwd_weight (tile kernels on the adjoint filter) against torch autograd of the
    oracle's convolution (oracle/train.py:_conv)."""
    from pcgcv1_amd import _lib
    rng = np.random.default_rng(cin * 131 + cout * 7 + k + stride + D)
    B = 2
    kshape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
    kern = (rng.standard_normal(kshape) * 0.2).astype(np.float32)
    x = rng.standard_normal((B, D, D, D, cin)).astype(np.float32)
    Dout = 2 * D if tr else D // stride
    dz = rng.standard_normal((B, Dout, Dout, Dout, cout)).astype(np.float32)
    # oracle
    wt = {"l/kernel": torch.tensor(kern, requires_grad=True)}
    xt = torch.tensor(x).permute(0, 4, 1, 2, 3).requires_grad_(True)
    y = otrain._conv(wt, "l", xt, stride=stride, tconv=bool(tr))
    y.backward(torch.tensor(dz).permute(0, 4, 1, 2, 3))
    dx_ref = xt.grad.permute(0, 2, 3, 4, 1).numpy()
    dk_ref = wt["l/kernel"].grad.numpy()
    # device
    lib = _lib.hip()
    dev = torch.device("cuda:0")
    n = int(lib.pcgc_conv3d_bwd_workspace_bytes(cin, cout, k))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    xd, dzd, kd = (torch.tensor(a, device=dev) for a in (x, dz, kern))
    dxd = torch.empty_like(xd)
    gk = torch.empty_like(kd)
    gb = torch.empty(cout, device=dev)
    _lib.check(lib.pcgc_conv3d_bwd_data(_lib.dptr(dzd), _lib.dptr(kd), _lib.dptr(dxd), B, D, cin, cout, k, stride, tr,
                                        _lib.dptr(ws), n, _lib.stream()), "bwd_data")
    torch.cuda.synchronize()
    _lib.check(lib.pcgc_conv3d_bwd_weight(_lib.dptr(xd), _lib.dptr(dzd), _lib.dptr(gk), _lib.dptr(gb), B, D, cin, cout, k,
                                          stride, tr, _lib.dptr(ws), n, _lib.stream()), "bwd_weight")
    torch.cuda.synchronize()
    sx, sk = float(np.abs(dx_ref).max()), float(np.abs(dk_ref).max())
    assert float(np.abs(dxd.cpu().numpy() - dx_ref).max()) <= 2e-5 * sx
    assert float(np.abs(gk.cpu().numpy() - dk_ref).max()) <= 1e-4 * sk
    np.testing.assert_allclose(gb.cpu().numpy(), dz.sum((0, 1, 2, 3)), rtol=1e-4, atol=1e-3)


def test_checkpoint_save_restore_resumes_bit_exactly(tmp_path):
    """Trainer.save / restore through the TensorFlow tensor-bundle files: a resumed run continues exactly."""
    w, x, ny, nz = _setup(seed=8)
    a = Trainer(w, alpha=0.75, beta=3.0, lr=1e-3)
    for _ in range(2):
        a.step(x, ny, nz)
    d = str(tmp_path / "ck")
    assert a.save(d).endswith("ckpt-2")
    a.step(x, ny, nz)
    b = Trainer(synthetic.make_weights(seed=99, profile="dense"), alpha=0.75, beta=3.0, lr=1e-3)
    b.restore(d)
    assert b.t == 2
    b.step(x, ny, nz)
    wa, wb = a.weights(), b.weights()
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    # the saved model loads through the codec's loader too
    from pcgcv1_amd import checkpoint
    got = checkpoint.load(d)
    assert sorted(got) == sorted(w)


@pytest.mark.parametrize("name", ["model_simple", "model_voxception"])
def test_train_factorized_gradients_match_autograd(name):
    """train_factorized.py step: loss terms and every parameter gradient of the autoencoder + factorized
    prior against torch autograd, for both model modules."""
    from pcgcv1_amd.train_factorized import Trainer as FTrainer
    rng = np.random.default_rng(17)
    B, cs = 2, 16
    x = synthetic.make_cubes(seed=17, n_cubes=B, cube_size=cs, occupancy=0.06)
    if name == "model_simple":
        w = synthetic.make_weights_simple(seed=17)
        lat = (B, cs // 8, cs // 8, cs // 8, 32)
    else:
        full = synthetic.make_weights(seed=17, profile="dense")
        w = {k: v for k, v in full.items() if k.startswith(("analysis_transform/", "synthesis_transform/"))}
        w.update({k: v for k, v in synthetic.make_weights_simple(seed=17).items() if k.startswith("estimator/")})
        w = {k: (v[:16] if k.startswith("estimator/") else v) for k, v in w.items()}          # 16 latent channels
        lat = (B, cs // 4, cs // 4, cs // 4, 16)
    ny = (rng.random(lat) - 0.5).astype(np.float32)
    terms_ref, leaves = otrain.forward_loss_factorized(w, x, ny, 2.0, 3.0, model=name)
    tr = FTrainer(w, model=name, alpha=2.0, beta=3.0, lr=1e-4)
    terms = tr.forward_backward(x, ny)
    for k in ("loss", "bpp", "empty", "full"):
        assert abs(terms[k] - terms_ref[k]) <= 2e-4 * max(1.0, abs(terms_ref[k])), (k, terms[k], terms_ref[k])
    for pname, leaf in leaves.items():
        g_ref = leaf.grad.numpy()
        g = tr.g[pname].cpu().numpy()
        scale = float(np.abs(g_ref).max())
        assert scale > 0, pname
        assert float(np.abs(g - g_ref).max()) / scale < 5e-3, pname
    first = tr.step(x, ny)["loss"]
    for _ in range(5):
        last = tr.step(x, ny)["loss"]
    assert np.isfinite(last) and last < first


def test_train_hyper_driver_cli(tmp_path, monkeypatch):
    """The training driver with the reference's flags: a few iterations on synthetic 16^3 cubes, checkpoint written in
    the TF format under checkpoints/<prefix>hyper|a..b../ (the reference's directory name, train_hyper.py:271-272), resumed
    by a second invocation; --reset_optimizer as the reference means it (107-121): 0 keeps Adam out of the checkpoint."""
    from pcgcv1_amd import tf_bundle, train_hyper
    monkeypatch.chdir(tmp_path)
    args = ["--alpha=0.75", "--beta=3", "--lr=1e-4", "--batch_size=2", "--cube_size=16", "--display_step=2", "--save_step=3", "--prefix=t_"]
    train_hyper.main(args + ["--num_iteration=4"])
    d = tmp_path / "checkpoints" / "t_hyper|a0.75b3.00"
    assert tf_bundle.latest_checkpoint(str(d)).endswith("ckpt-4")
    train_hyper.main(args + ["--num_iteration=6"])                     # resumes at step 4
    assert tf_bundle.latest_checkpoint(str(d)).endswith("ckpt-6")
    raw = tf_bundle.read_bundle(tf_bundle.latest_checkpoint(str(d)))
    assert int(np.asarray(raw["global_step"]).reshape(-1)[0]) == 6
    assert not any(".OPTIMIZER_SLOT" in k for k in raw)                # default --reset_optimizer=0: no optimizer in the file
    train_hyper.main(args + ["--num_iteration=8", "--reset_optimizer=1", "--prefix=o_"])
    raw = tf_bundle.read_bundle(tf_bundle.latest_checkpoint(str(tmp_path / "checkpoints" / "o_hyper|a0.75b3.00")))
    assert "analysis_transform/conv_in/kernel/.OPTIMIZER_SLOT/main_optimizer/m" in raw


def test_evaluate_matches_the_oracle_eval_forward():
    """Trainer.evaluate = the held-out evaluation batch of the training loop (train_hyper.py:126-162): rounded latents,
    bpp terms and IoU after the adaptive top-k, against oracle.transform.rate_terms / classify_metrics."""
    from oracle import points as opoints
    from oracle import transform as otransform
    w, x, _, _ = _setup(seed=9, B=2, cs=16)
    tr = Trainer(w)
    ev = tr.evaluate(x)
    assert ev == tr.evaluate(x)                              # no noise, no state: bit-repeatable
    ref = otransform.rate_terms(w, x)
    assert abs(ev["bpp_y"] - ref["bpp_y"]) < 1e-3 * max(1.0, abs(ref["bpp_y"]))
    assert abs(ev["bpp_z"] - ref["bpp_z"]) < 1e-3 * max(1.0, abs(ref["bpp_z"]))
    nums = x.reshape(x.shape[0], -1).sum(axis=1).astype(np.int64)
    mask = opoints.select_voxels(ref["x_tilde"], nums, 1.0)
    iou = float(otransform.classify_metrics(mask, x)[2])
    assert abs(ev["IoU"] - iou) < 2e-2                       # a handful of voxels near the k-th value may swap
    assert ev["num_points"] == float(x.sum())


def test_driver_trains_on_a_generated_dataset_with_held_out_eval(tmp_path, monkeypatch):
    """generate_dataset -> train_hyper on the cube files: 1/9 held out, evaluated before each checkpoint, scalars logged
    in the reference's four summaries (bpp_ae, bpp_hyper, bpp, IoU) for the train and eval writers."""
    import json
    from pcgcv1_amd import generate_dataset, train_hyper
    from pcgcv1_amd.dataprocess import inout_points as iop
    monkeypatch.chdir(tmp_path)
    (tmp_path / "ply").mkdir()
    for i in range(2):
        iop.write_ply_data(str(tmp_path / "ply" / ("c%d.ply" % i)), synthetic.make_cloud(seed=20 + i, res=64, n_shells=3, rmin=0.2, rmax=0.45))
    files = generate_dataset.generate_dataset(str(tmp_path / "ply"), str(tmp_path / "cubes"), 1e6, cube_size=16, seed=1)
    assert len(files) >= 18
    held, train = train_hyper.split_file_list(sorted(files))
    assert len(held) == len(files) // 9 and len(held) + len(train) == len(files)
    args = ["--alpha=0.75", "--beta=3", "--lr=1e-4", "--batch_size=2", "--cube_size=16", "--display_step=2", "--save_step=2",
            "--prefix=d_", "--data=" + str(tmp_path / "cubes" / "*.npy"), "--num_iteration=4"]
    train_hyper.main(args)
    for name, steps in (("d_hyper_a0.75b3.00", [2, 4]), ("d_hyper_eval_a0.75b3.00", [2, 4])):      # train_hyper.py:289-296
        rows = [json.loads(l) for l in open(tmp_path / "logs" / name / "scalars.jsonl")]
        assert [r["step"] for r in rows] == steps
        for r in rows:
            assert set(r) == {"step", "bpp_ae", "bpp_hyper", "bpp", "IoU"}
            assert np.isfinite(r["bpp"]) and abs(r["bpp"] - r["bpp_ae"] - r["bpp_hyper"]) < 1e-9 and 0.0 <= r["IoU"] <= 1.0


def test_training_plan_matches_the_per_layer_entry_points():
    """csrc/train_plan.hip: forward, bwd-data and bwd-weight through the plan (filters prepared for all layers in two
    launches, weight-gradient reductions batched) are bit-identical to pcgc_conv3d_fwd / _bwd_data_fused / _bwd_weight."""
    import ctypes
    from pcgcv1_amd import _lib
    from pcgcv1_amd.models.model_voxception import conv3d
    from pcgcv1_amd.train_hyper import _TrainLayer
    lib = _lib.hip()
    dev = _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(3)
    #        cin cout k stride transposed bias D
    shapes = [(16, 4, 3, 1, 0, True, 16), (4, 8, 1, 1, 0, True, 16), (16, 32, 3, 2, 0, True, 16), (32, 16, 3, 2, 1, True, 8),
              (64, 64, 3, 1, 0, False, 16), (1, 16, 3, 1, 0, True, 16), (16, 1, 3, 1, 0, True, 16), (8, 8, 3, 1, 0, True, 32)]
    B = 2
    ks, gks, gbs = [], [], []
    arr = (_TrainLayer * len(shapes))()
    for i, (cin, cout, k, stride, tr, bias, D) in enumerate(shapes):
        shape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
        ks.append((torch.randn(shape, generator=g) * 0.2).to(dev))
        gks.append(torch.zeros(shape, device=dev))
        gbs.append(torch.zeros(cout, device=dev) if bias else None)
        arr[i].kernel, arr[i].dkernel = ks[i].data_ptr(), gks[i].data_ptr()
        arr[i].dbias = gbs[i].data_ptr() if bias else None
        arr[i].Cin, arr[i].Cout, arr[i].ksize, arr[i].stride, arr[i].transposed = cin, cout, k, stride, tr
    plan = ctypes.c_void_p()
    _lib.check(lib.pcgc_train_plan_create(ctypes.cast(arr, ctypes.c_void_p), len(shapes), ctypes.byref(plan)))
    assert lib.pcgc_train_plan_layers(plan) == len(shapes)
    try:
        for rep in range(2):                                  # second round: right-sized pool, filters changed in place
            for kk in ks:
                kk.mul_(1.0 + 0.5 * rep)
            _lib.check(lib.pcgc_train_plan_prepare(plan, _lib.stream()))
            want = []
            for i, (cin, cout, k, stride, tr, bias, D) in enumerate(shapes):
                x = torch.relu(torch.randn((B, D, D, D, cin), generator=g)).to(dev)
                b = (torch.randn(cout, generator=g) * 0.1).to(dev) if bias else None
                y_ref = conv3d(x, ks[i], b, stride=stride, transposed=bool(tr), relu=True)
                y = torch.empty_like(y_ref)
                _lib.check(lib.pcgc_train_conv_fwd(plan, i, _lib.dptr(x), _lib.dptr(b), _lib.dptr(y), B, D, 1, _lib.stream()))
                assert torch.equal(y, y_ref), shapes[i]
                dz = torch.randn(y.shape, generator=g).to(dev)
                add_to = torch.randn(x.shape, generator=g).to(dev)
                ws = torch.empty(int(lib.pcgc_conv3d_bwd_workspace_bytes(cin, cout, k)), dtype=torch.uint8, device=dev)
                dx_ref, dx = torch.empty_like(x), torch.empty_like(x)
                _lib.check(lib.pcgc_conv3d_bwd_data_fused(_lib.dptr(dz), _lib.dptr(ks[i]), _lib.dptr(dx_ref), _lib.dptr(x), _lib.dptr(add_to),
                                                          B, D, cin, cout, k, stride, tr, _lib.dptr(ws), ws.numel(), _lib.stream()))
                _lib.check(lib.pcgc_train_conv_bwd_data(plan, i, _lib.dptr(dz), _lib.dptr(dx), _lib.dptr(x), _lib.dptr(add_to), B, D,
                                                        _lib.stream()))
                assert torch.equal(dx, dx_ref), shapes[i]
                gk_ref, gb_ref = torch.empty_like(ks[i]), (torch.empty(cout, device=dev) if bias else None)
                _lib.check(lib.pcgc_conv3d_bwd_weight(_lib.dptr(x), _lib.dptr(dz), _lib.dptr(gk_ref), _lib.dptr(gb_ref), B, D, cin, cout, k,
                                                      stride, tr, _lib.dptr(ws), ws.numel(), _lib.stream()))
                _lib.check(lib.pcgc_train_conv_bwd_weight(plan, i, _lib.dptr(x), _lib.dptr(dz), B, D, _lib.stream()))
                want.append((gk_ref, gb_ref))
            _lib.check(lib.pcgc_train_plan_finish_weights(plan, _lib.stream()))
            for i, (gk_ref, gb_ref) in enumerate(want):
                assert torch.equal(gks[i], gk_ref), shapes[i]
                if gb_ref is not None:
                    assert torch.equal(gbs[i], gb_ref), shapes[i]
    finally:
        lib.pcgc_train_plan_destroy(plan)


@pytest.mark.parametrize("B,D", [(8, 16), (2, 32), (24, 16), (2, 8)])
def test_two_layer_entry_points_match_the_single_calls(B, D):
    """pcgc_train_conv_fwd_pair / _bwd_data_pair / _fwd_merge / _bwd_data_chain on the shapes of a C = 64 block against the
    single calls they stand for, bit for bit: a small launch at 16^3 and at 32^3 (the two-layer kernels), a large one (24 cubes:
    not a small launch any more) and 8^3 (no MFMA tile geometry) where they run the single calls inside."""
    import ctypes
    from pcgcv1_amd import _lib
    from pcgcv1_amd.train_hyper import _TrainLayer
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(B * 100 + D)
    shapes = [(64, 16, 3), (64, 16, 1), (16, 32, 3), (16, 16, 3), (16, 32, 1)]                    # conv1_1, conv2_1, conv1_2, conv2_2, conv2_3
    ks = [(torch.randn((k, k, k, ci, co), generator=g) * 0.1).to(dev) for ci, co, k in shapes]
    gks = [torch.zeros_like(k_) for k_ in ks]
    gbs = [torch.zeros(co, device=dev) for _, co, _ in shapes]
    bs = [torch.randn(co, generator=g).to(dev) for _, co, _ in shapes]
    arr = (_TrainLayer * len(shapes))()
    for i, (ci, co, k) in enumerate(shapes):
        arr[i].kernel, arr[i].dkernel, arr[i].dbias = ks[i].data_ptr(), gks[i].data_ptr(), gbs[i].data_ptr()
        arr[i].Cin, arr[i].Cout, arr[i].ksize, arr[i].stride, arr[i].transposed = ci, co, k, 1, 0
    plan = ctypes.c_void_p()
    _lib.check(lib.pcgc_train_plan_create(ctypes.cast(arr, ctypes.c_void_p), len(shapes), ctypes.byref(plan)))
    st, P = _lib.stream(), _lib.dptr
    rnd = lambda c, relu=False: (torch.relu(torch.randn((B, D, D, D, c), generator=g)) if relu else torch.randn((B, D, D, D, c), generator=g)).to(dev)
    try:
        _lib.check(lib.pcgc_train_plan_prepare(plan, st))
        x, t11, t21 = rnd(64, True), rnd(16, True), rnd(16, True)
        fwd = lambda i, xin: (lambda y: (_lib.check(lib.pcgc_train_conv_fwd(plan, i, P(xin), P(bs[i]), P(y), B, D, 1, st)), y)[1])(torch.empty((B, D, D, D, shapes[i][1]), device=dev))
        # forward pairs: conv1_1 | conv2_1 on the block input, conv1_2 | conv2_2 on their outputs
        for (ia, ib, xa, xb) in ((0, 1, x, x), (2, 3, t11, t21)):
            ya, yb = torch.empty((B, D, D, D, shapes[ia][1]), device=dev), torch.empty((B, D, D, D, shapes[ib][1]), device=dev)
            _lib.check(lib.pcgc_train_conv_fwd_pair(plan, ia, ib, P(xa), P(xb), P(bs[ia]), P(bs[ib]), P(ya), P(yb), B, D, 1, 1, st))
            assert torch.equal(ya, fwd(ia, xa)) and torch.equal(yb, fwd(ib, xb)), (ia, ib)
        # conv2_3 with the block's merge
        t22, t12 = rnd(16, True), rnd(32, True)
        t23, out = torch.empty((B, D, D, D, 32), device=dev), torch.empty((B, D, D, D, 64), device=dev)
        _lib.check(lib.pcgc_train_conv_fwd_merge(plan, 4, P(t22), P(bs[4]), P(t23), 1, P(x), P(t12), P(out), 64, B, D, st))
        t23_ref, out_ref = fwd(4, t22), torch.empty_like(out)
        _lib.check(lib.pcgc_vrn_merge(P(x), P(t12), P(t23_ref), P(out_ref), x.numel() // 64, 64, st))
        assert torch.equal(t23, t23_ref) and torch.equal(out, out_ref)
        assert torch.equal(out, torch.relu(x + torch.cat([t12, t23_ref], dim=-1)))
        # reverse pair conv1_2^T | conv2_3^T (masked by the layers' inputs)
        dz12, dz23 = rnd(32), rnd(32)
        da, db = torch.empty_like(t11), torch.empty_like(t22)
        _lib.check(lib.pcgc_train_conv_bwd_data_pair(plan, 2, 4, P(dz12), P(dz23), P(da), P(db), P(t11), P(t22), B, D, st))
        ra, rb = torch.empty_like(t11), torch.empty_like(t22)
        _lib.check(lib.pcgc_train_conv_bwd_data(plan, 2, P(dz12), P(ra), P(t11), None, B, D, st))
        _lib.check(lib.pcgc_train_conv_bwd_data(plan, 4, P(dz23), P(rb), P(t22), None, B, D, st))
        assert torch.equal(da, ra) and torch.equal(db, rb) and float(da.abs().max()) > 0
        # reverse chain conv1_1^T, then conv2_1^T, in place on the skip connection's gradient; with and without the ReLU mask
        dt11, dt21 = rnd(16), rnd(16)
        for mask in (x, None):
            dpre = rnd(64)
            want = dpre.clone()
            _lib.check(lib.pcgc_train_conv_bwd_data(plan, 0, P(dt11), P(want), P(mask), P(want), B, D, st))
            _lib.check(lib.pcgc_train_conv_bwd_data(plan, 1, P(dt21), P(want), P(mask), P(want), B, D, st))
            _lib.check(lib.pcgc_train_conv_bwd_data_chain(plan, 0, 1, P(dt11), P(dt21), P(dpre), P(mask), B, D, st))
            assert torch.equal(dpre, want), mask is None
    finally:
        lib.pcgc_train_plan_destroy(plan)


@pytest.mark.parametrize("cin,cout,D,B", [(16, 4, 64, 2), (32, 8, 32, 3), (64, 16, 16, 2)])
def test_weight_gradient_pair_matches_the_single_calls(cin, cout, D, B):
    """pcgc_train_conv_bwd_weight_pair (conv1_1 3^3 and conv2_1 1^3 of a VRN block in one pass over the block input) against
    the two pcgc_train_conv_bwd_weight calls: the 3^3 layer bit for bit, the 1^3 layer (another summation order) within
    fp32 rounding of a float64 reference; the third shape has no fused kernel and takes the single calls."""
    import ctypes
    from pcgcv1_amd import _lib
    from pcgcv1_amd.train_hyper import _TrainLayer
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(cin + D)
    shapes = [(cin, cout, 3), (cin, cout, 1)] * 2             # layers 0, 1: the pair call; 2, 3: the single calls
    ks = [(torch.randn((k, k, k, ci, co), generator=g) * 0.2).to(dev) for ci, co, k in shapes]
    gks = [torch.zeros_like(k_) for k_ in ks]
    gbs = [torch.zeros(cout, device=dev) for _ in shapes]
    arr = (_TrainLayer * len(shapes))()
    for i, (ci, co, k) in enumerate(shapes):
        arr[i].kernel, arr[i].dkernel, arr[i].dbias = ks[i].data_ptr(), gks[i].data_ptr(), gbs[i].data_ptr()
        arr[i].Cin, arr[i].Cout, arr[i].ksize, arr[i].stride, arr[i].transposed = ci, co, k, 1, 0
    plan = ctypes.c_void_p()
    _lib.check(lib.pcgc_train_plan_create(ctypes.cast(arr, ctypes.c_void_p), len(shapes), ctypes.byref(plan)))
    try:
        x = torch.relu(torch.randn((B, D, D, D, cin), generator=g)).to(dev)
        dz3 = torch.randn((B, D, D, D, cout), generator=g).to(dev)
        dz1 = torch.randn((B, D, D, D, cout), generator=g).to(dev)
        for rep in range(2):
            _lib.check(lib.pcgc_train_plan_prepare(plan, _lib.stream()))
            _lib.check(lib.pcgc_train_conv_bwd_weight_pair(plan, 0, 1, _lib.dptr(x), _lib.dptr(dz3), _lib.dptr(dz1), B, D, _lib.stream()))
            _lib.check(lib.pcgc_train_conv_bwd_weight(plan, 2, _lib.dptr(x), _lib.dptr(dz3), B, D, _lib.stream()))
            _lib.check(lib.pcgc_train_conv_bwd_weight(plan, 3, _lib.dptr(x), _lib.dptr(dz1), B, D, _lib.stream()))
            _lib.check(lib.pcgc_train_plan_finish_weights(plan, _lib.stream()))
            assert torch.equal(gks[0], gks[2]) and torch.equal(gbs[0], gbs[2])
            ref1 = torch.einsum("bdhwi,bdhwo->io", x.double(), dz1.double()).reshape(1, 1, 1, cin, cout)
            tol = 2e-6 * float(ref1.abs().max()) * (B * D ** 3) ** 0.5
            assert float((gks[1].double() - ref1).abs().max()) <= tol and float((gks[3].double() - ref1).abs().max()) <= tol
            assert float((gbs[1].double() - dz1.double().sum((0, 1, 2, 3))).abs().max()) <= tol
            if rep == 0:
                first = (gks[1].clone(), gbs[1].clone())
            else:                                           # fixed summation order: the same bits every time
                assert torch.equal(gks[1], first[0]) and torch.equal(gbs[1], first[1])
    finally:
        lib.pcgc_train_plan_destroy(plan)


def test_vrn_bwd_split_matches_relu_bwd():
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(5)
    nvox, C = 4099, 16
    dout, out = torch.randn((nvox, C), generator=g).to(dev), torch.randn((nvox, C), generator=g).to(dev)
    t12, t23 = torch.randn((nvox, C // 2), generator=g).to(dev), torch.randn((nvox, C // 2), generator=g).to(dev)
    for premasked in (0, 1):
        dpre, dz12, dz23 = torch.full_like(dout, 7.0), torch.empty_like(t12), torch.empty_like(t23)
        _lib.check(lib.pcgc_vrn_bwd_split(_lib.dptr(dout), _lib.dptr(out), _lib.dptr(t12), _lib.dptr(t23),
                                          None if premasked else _lib.dptr(dpre), _lib.dptr(dz12), _lib.dptr(dz23), nvox, C, premasked,
                                          _lib.stream()))
        ref = dout if premasked else dout * (out > 0)
        if not premasked:
            assert torch.equal(dpre, ref)
        assert torch.equal(dz12, ref[:, :C // 2] * (t12 > 0)) and torch.equal(dz23, ref[:, C // 2:] * (t23 > 0))


@pytest.mark.parametrize("geom", [(64, 16), (32, 32)])
def test_vrn_sign_bits_match_the_full_tensors(geom):
    """pcgc_vrn_fwd_train_signs / pcgc_vrn_bwd_split_signs against pcgc_vrn_fwd_train / pcgc_vrn_bwd_split on the same
    block: identical saved tensors, sign bits == (pre > 0) exactly, identical dpre / dz12 / dz23."""
    import ctypes
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    assert lib.pcgc_vrn_fwd_train_signs_supported(64, 16) == 1 and lib.pcgc_vrn_fwd_train_signs_supported(32, 32) == 1
    assert lib.pcgc_vrn_fwd_train_signs_supported(16, 64) == 0
    g = torch.Generator(device="cpu").manual_seed(31)
    D, C = geom
    B, Q, H = (2 if D == 64 else 3), C // 4, C // 2
    shapes = [(3, 3, 3, C, Q), (Q,), (3, 3, 3, Q, H), (H,), (1, 1, 1, C, Q), (Q,), (3, 3, 3, Q, Q), (Q,), (1, 1, 1, Q, H), (H,)]
    params = [(torch.randn(sh, generator=g) * (0.15 if len(sh) > 1 else 0.05) * (16.0 / C) ** 0.5).to(dev) for sh in shapes]
    arr = (ctypes.c_void_p * 10)(*[p.data_ptr() for p in params])
    x = torch.relu(torch.randn((B, D, D, D, C), generator=g)).to(dev)
    q = (B, D, D, D, Q)
    a = [torch.empty(q, device=dev) for _ in range(3)] + [torch.empty_like(x), torch.empty_like(x)]
    b = [torch.empty(q, device=dev) for _ in range(3)] + [torch.empty((B, D, D, D), dtype=torch.int32, device=dev), torch.empty_like(x)]
    _lib.check(lib.pcgc_vrn_fwd_train(_lib.dptr(x), ctypes.cast(arr, ctypes.c_void_p), *[_lib.dptr(t) for t in a], B, D, C, _lib.stream()))
    _lib.check(lib.pcgc_vrn_fwd_train_signs(_lib.dptr(x), ctypes.cast(arr, ctypes.c_void_p), *[_lib.dptr(t) for t in b], B, D, C, _lib.stream()))
    for i in (0, 1, 2, 4):
        assert torch.equal(a[i], b[i]), i
    pre, signs = a[3], b[3]
    assert 0.05 < float((pre > 0).float().mean()) < 0.95
    for c in range(C):
        assert torch.equal(((signs >> c) & 1).bool(), pre[..., c] > 0), c
    if C == 16:              # the 64^3 blocks' words also carry the masks of the block's reverse: t22 > 0, t11 > 0, t21 > 0
        for i in range(4):
            assert torch.equal(((signs >> (16 + i)) & 1).bool(), a[2][..., i] > 0), ("t22", i)
            assert torch.equal(((signs >> (20 + i)) & 1).bool(), a[0][..., i] > 0), ("t11", i)
            assert torch.equal(((signs >> (24 + i)) & 1).bool(), a[1][..., i] > 0), ("t21", i)
        assert int((signs >> 28).abs().max()) == 0
    dout, nvox = torch.randn(x.shape, generator=g).to(dev), B * D * D * D
    for premasked in (0, 1):
        ra = [torch.full_like(x, 7.0), torch.empty((B, D, D, D, H), device=dev), torch.empty((B, D, D, D, H), device=dev)]
        rb = [torch.full_like(x, 7.0), torch.empty((B, D, D, D, H), device=dev), torch.empty((B, D, D, D, H), device=dev)]
        _lib.check(lib.pcgc_vrn_bwd_split(_lib.dptr(dout), _lib.dptr(a[4]), _lib.dptr(pre), None, None if premasked else _lib.dptr(ra[0]),
                                          _lib.dptr(ra[1]), _lib.dptr(ra[2]), nvox, C, premasked, _lib.stream()))
        _lib.check(lib.pcgc_vrn_bwd_split_signs(_lib.dptr(dout), _lib.dptr(a[4]), _lib.dptr(signs), None if premasked else _lib.dptr(rb[0]),
                                                _lib.dptr(rb[1]), _lib.dptr(rb[2]), nvox, C, premasked, _lib.stream()))
        for u, v in zip(ra, rb):
            assert torch.equal(u, v)


def test_fused_vrn_forward_matches_the_layerwise_step_at_64():
    """pcgc_vrn_fwd_train (the 4x4x1-MFMA row kernels on the training tensors: D = 64 / C = 16 and D = 32 / C = 32 blocks) against the same
    step run layer by layer: every saved tensor of a block, the loss terms and all gradients."""
    import ctypes
    from pcgcv1_amd import _lib
    from pcgcv1_amd.models import spec
    w = synthetic.make_weights(seed=11, profile="dense")
    x = synthetic.make_cubes(seed=11, n_cubes=1, cube_size=64)
    rng = np.random.default_rng(11)
    ny = (rng.random((1, 16, 16, 16, 16)) - 0.5).astype(np.float32)
    nz = (rng.random((1, 8, 8, 8, 8)) - 0.5).astype(np.float32)
    tr = Trainer(w)
    lib = _lib.hip()
    assert lib.pcgc_vrn_fwd_train_supported(64, 16) == 1 and lib.pcgc_vrn_fwd_train_supported(32, 32) == 1
    assert lib.pcgc_vrn_fwd_train_supported(16, 64) == 0 and lib.pcgc_vrn_fwd_train_supported(32, 16) == 0
    # one block of each fused stage, tensor by tensor
    table = spec.NETS["analysis_transform"]()
    tr._prepare()
    for D, C, first in ((64, 16, "vrn1_1/conv1_1"), (32, 32, "vrn2_1/conv1_1")):
        i0 = [l.name for l in table].index(first)
        layers = table[i0:i0 + 5]
        xin = torch.relu(torch.randn((2, D, D, D, C), generator=torch.Generator().manual_seed(D))).to(tr.dev)
        tr.fused_vrn = True
        out_f, cf = tr._vrn("analysis_transform", layers, xin)
        tr.fused_vrn = False
        out_l, cl = tr._vrn("analysis_transform", layers, xin)
        tr.fused_vrn = True
        assert cf[8] is not None and cl[8] is None
        scale = float(out_l.abs().max())
        assert float((out_f - out_l).abs().max()) < 2e-5 * max(1.0, scale), (D, C)
        for kf, kl in zip(cf[3:8], cl[3:8]):                    # k11, k12, k21, k22, k23: inputs (and outputs where kept)
            assert float((kf[2] - kl[2]).abs().max()) < 2e-5 * max(1.0, float(kl[2].abs().max())), (D, C, kl[1].name)
        pre_l = torch.cat([cl[4][3], cl[7][3]], dim=-1)
        if cf[8].dtype == torch.int32:                          # only the signs were kept: bit c = (pre[c] > 0)
            bits = torch.stack([(cf[8] >> c) & 1 for c in range(C)], dim=-1).bool()
            differ = bits != (pre_l > 0)                        # the two paths sum in different orders: a value within rounding of 0 may flip
            assert float(differ.float().mean()) < 1e-5 and float(pre_l[differ].abs().max() if differ.any() else 0.0) < 1e-5, (D, C)
        else:
            assert float((cf[8] - pre_l).abs().max()) < 2e-5 * max(1.0, float(pre_l.abs().max())), (D, C)
    # whole step
    a = tr.forward_backward(x, ny, nz)
    g_f = tr.flat_g.clone()
    tr.fused_vrn = False
    b = tr.forward_backward(x, ny, nz)
    g_l = tr.flat_g.clone()
    for k in ("loss", "bpp_y", "bpp_z", "empty", "full"):
        assert abs(a[k] - b[k]) < 1e-4 * max(1.0, abs(b[k])), k
    assert float((g_f - g_l).abs().max()) < 2e-3 * float(g_l.abs().max())
    assert float((g_f - g_l).norm()) < 1e-3 * float(g_l.norm())


@pytest.mark.parametrize("geom", [(64, 16), (32, 32)])
@pytest.mark.parametrize("mask", [True, False])
def test_vrn_bwd_input_matches_conv_transpose(mask, geom):
    """pcgc_vrn_bwd_input (one row-kernel pass for the block input's three gradient contributions) against
    [x > 0] * (dpre + conv_transpose3d(dt11, w11) + conv_transpose3d(dt21, w21)) in plain PyTorch fp32 on the host,
    in place on dpre, cube faces included."""
    import torch.nn.functional as F
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    assert lib.pcgc_vrn_bwd_input_supported(64, 16) == 1 and lib.pcgc_vrn_bwd_input_supported(32, 32) == 1 and lib.pcgc_vrn_bwd_input_supported(16, 64) == 0
    g = torch.Generator(device="cpu").manual_seed(21)
    D, C = geom
    B, Q = (2 if D == 64 else 3), C // 4
    dt11, dt21 = torch.randn((B, D, D, D, Q), generator=g), torch.randn((B, D, D, D, Q), generator=g)
    dpre, x = torch.randn((B, D, D, D, C), generator=g), torch.randn((B, D, D, D, C), generator=g)
    w11 = torch.randn((3, 3, 3, C, Q), generator=g) * 0.1
    w21 = torch.randn((1, 1, 1, C, Q), generator=g) * 0.3
    ncdhw = lambda t: t.permute(0, 4, 1, 2, 3)
    ref = ncdhw(dpre) + F.conv_transpose3d(ncdhw(dt11), w11.permute(4, 3, 0, 1, 2), padding=1) \
        + F.conv_transpose3d(ncdhw(dt21), w21.permute(4, 3, 0, 1, 2))
    ref = ref.permute(0, 2, 3, 4, 1)
    if mask:
        ref = ref * (x > 0)
    d = [t.to(dev).contiguous() for t in (dt11, dt21, dpre, x, w11, w21)]
    _lib.check(lib.pcgc_vrn_bwd_input(_lib.dptr(d[0]), _lib.dptr(d[1]), _lib.dptr(d[2]), _lib.dptr(d[3]) if mask else None, _lib.dptr(d[4]),
                                      _lib.dptr(d[5]), _lib.dptr(d[2]), B, D, C, _lib.stream()), "pcgc_vrn_bwd_input")
    got = d[2].cpu()
    assert float((got - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
    again = dpre.to(dev)
    _lib.check(lib.pcgc_vrn_bwd_input(_lib.dptr(d[0]), _lib.dptr(d[1]), _lib.dptr(again), _lib.dptr(d[3]) if mask else None, _lib.dptr(d[4]),
                                      _lib.dptr(d[5]), _lib.dptr(again), B, D, C, _lib.stream()), "pcgc_vrn_bwd_input")
    assert torch.equal(again.cpu(), got)                                    # run to run


@pytest.mark.parametrize("geom", [(64, 16), (32, 32)])
def test_vrn_bwd_tail_matches_conv_transpose(geom):
    """pcgc_vrn_bwd_tail (the block's three inner bwd-data passes in one row kernel) against plain PyTorch fp32 on the host:
    dt11 = [t11 > 0] conv1_2^T(dz12), dt22 = [t22 > 0] conv2_3^T(dz23), dt21 = [t21 > 0] conv2_2^T(dt22); cube faces included."""
    import torch.nn.functional as F
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    assert lib.pcgc_vrn_bwd_tail_supported(64, 16) == 1 and lib.pcgc_vrn_bwd_tail_supported(32, 32) == 1 and lib.pcgc_vrn_bwd_tail_supported(16, 64) == 0
    g = torch.Generator(device="cpu").manual_seed(41)
    D, C = geom
    B, Q, H = (2 if D == 64 else 3), C // 4, C // 2
    dz12, dz23 = torch.randn((B, D, D, D, H), generator=g), torch.randn((B, D, D, D, H), generator=g)
    t11, t21, t22 = (torch.randn((B, D, D, D, Q), generator=g) for _ in range(3))
    w12 = torch.randn((3, 3, 3, Q, H), generator=g) * 0.1
    w22 = torch.randn((3, 3, 3, Q, Q), generator=g) * 0.15
    w23 = torch.randn((1, 1, 1, Q, H), generator=g) * 0.3
    nc = lambda t: t.permute(0, 4, 1, 2, 3)
    nl = lambda t: t.permute(0, 2, 3, 4, 1)
    r11 = nl(F.conv_transpose3d(nc(dz12), w12.permute(4, 3, 0, 1, 2), padding=1)) * (t11 > 0)
    r22 = nl(F.conv_transpose3d(nc(dz23), w23.permute(4, 3, 0, 1, 2))) * (t22 > 0)
    r21 = nl(F.conv_transpose3d(nc(r22), w22.permute(4, 3, 0, 1, 2), padding=1)) * (t21 > 0)
    d = [t.to(dev).contiguous() for t in (dz12, dz23, t11, t21, t22, w12, w22, w23)]
    outs = [torch.full((B, D, D, D, Q), 7.0, device=dev) for _ in range(3)]
    def run(o):
        _lib.check(lib.pcgc_vrn_bwd_tail(*[_lib.dptr(t) for t in d], *[_lib.dptr(t) for t in o], B, D, C, _lib.stream()), "pcgc_vrn_bwd_tail")
    run(outs)
    for got, ref, name in zip(outs, (r11, r21, r22), ("dt11", "dt21", "dt22")):
        assert float((got.cpu() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), name
    again = [torch.empty_like(o) for o in outs]
    run(again)
    for a_, b_ in zip(outs, again):
        assert torch.equal(a_, b_)                                            # run to run


@pytest.mark.parametrize("geom", [(64, 16)])
def test_vrn_bwd_tail_split_equals_split_then_tail(geom):
    """pcgc_vrn_bwd_tail_split == pcgc_vrn_bwd_split_signs (premasked) followed by pcgc_vrn_bwd_tail, bit for bit: the
    masks are elementwise, so making dz12 / dz23 inside the row kernel changes no sum."""
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    assert lib.pcgc_vrn_bwd_tail_split_supported(64, 16) == 1 and lib.pcgc_vrn_bwd_tail_split_supported(32, 32) == 0
    g = torch.Generator(device="cpu").manual_seed(43)
    D, C = geom
    B, Q, H = (2 if D == 64 else 3), C // 4, C // 2
    dout = torch.randn((B, D, D, D, C), generator=g).to(dev)
    signs = torch.randint(0, 1 << 16, (B, D, D, D), generator=g, dtype=torch.int32).to(dev)
    t11, t21, t22 = (torch.randn((B, D, D, D, Q), generator=g).to(dev) for _ in range(3))
    # the one-pass kernel takes the masks t22 > 0, t11 > 0, t21 > 0 from bits 16-19 / 20-23 / 24-27 of the words (as the
    # forward kernel writes them) and does not read the tensors
    for base, t in ((16, t22), (20, t11), (24, t21)):
        for i in range(4):
            signs |= (t[..., i] > 0).to(torch.int32) << (base + i)
    w12 = (torch.randn((3, 3, 3, Q, H), generator=g) * 0.1).to(dev)
    w22 = (torch.randn((3, 3, 3, Q, Q), generator=g) * 0.15).to(dev)
    w23 = (torch.randn((1, 1, 1, Q, H), generator=g) * 0.3).to(dev)
    half = (B, D, D, D, H)
    a = [torch.empty(half, device=dev), torch.empty(half, device=dev)] + [torch.empty_like(t11) for _ in range(3)]
    b = [torch.full(half, 7.0, device=dev), torch.full(half, 7.0, device=dev)] + [torch.full_like(t11, 7.0) for _ in range(3)]
    _lib.check(lib.pcgc_vrn_bwd_split_signs(_lib.dptr(dout), None, _lib.dptr(signs), None, _lib.dptr(a[0]), _lib.dptr(a[1]), B * D * D * D, C, 1,
                                            _lib.stream()))
    _lib.check(lib.pcgc_vrn_bwd_tail(_lib.dptr(a[0]), _lib.dptr(a[1]), _lib.dptr(t11), _lib.dptr(t21), _lib.dptr(t22), _lib.dptr(w12),
                                     _lib.dptr(w22), _lib.dptr(w23), _lib.dptr(a[2]), _lib.dptr(a[3]), _lib.dptr(a[4]), B, D, C, _lib.stream()))
    _lib.check(lib.pcgc_vrn_bwd_tail_split(_lib.dptr(dout), _lib.dptr(signs), _lib.dptr(t11), _lib.dptr(t21), _lib.dptr(t22), _lib.dptr(w12),
                                           _lib.dptr(w22), _lib.dptr(w23), *[_lib.dptr(t) for t in b], B, D, C, _lib.stream()))
    for u, v, name in zip(a, b, ("dz12", "dz23", "dt11", "dt21", "dt22")):
        assert torch.equal(u, v), name


def test_debug_switch_refuses_sign_words_without_the_relu_masks():
    """PCGC_DEBUG_SIGNS=1 (read once per process, hence the child): pcgc_vrn_bwd_tail_split takes (t22 > 0), (t11 > 0), (t21 > 0)
    from bits 16-27 of the sign words and never reads the tensors; words in the plain "bit c = pre[c] > 0" form would zero
    dt11 / dt21 / dt22 silently.  With the switch on such words are refused with an error, words that carry the masks pass."""
    import subprocess
    import sys
    code = r"""
import sys, torch
sys.path.insert(0, %r)
from pcgcv1_amd import _lib
lib, dev = _lib.hip(), _lib.require_gpu()
g = torch.Generator(device="cpu").manual_seed(3)
B, D, C, Q, H = 1, 64, 16, 4, 8
dout = torch.randn((B, D, D, D, C), generator=g).to(dev)
plain = torch.randint(0, 1 << 16, (B, D, D, D), generator=g, dtype=torch.int32).to(dev)
t11, t21, t22 = (torch.randn((B, D, D, D, Q), generator=g).to(dev) for _ in range(3))
full = plain.clone()
for base, t in ((16, t22), (20, t11), (24, t21)):
    for i in range(4):
        full |= (t[..., i] > 0).to(torch.int32) << (base + i)
w12, w22, w23 = torch.randn((3, 3, 3, Q, H)).to(dev), torch.randn((3, 3, 3, Q, Q)).to(dev), torch.randn((1, 1, 1, Q, H)).to(dev)
outs = [torch.empty((B, D, D, D, H), device=dev) for _ in range(2)] + [torch.empty_like(t11) for _ in range(3)]
def call(signs):
    return lib.pcgc_vrn_bwd_tail_split(_lib.dptr(dout), _lib.dptr(signs), _lib.dptr(t11), _lib.dptr(t21), _lib.dptr(t22), _lib.dptr(w12),
                                       _lib.dptr(w22), _lib.dptr(w23), *[_lib.dptr(t) for t in outs], B, D, C, _lib.stream())
assert call(full) == 0
rc = call(plain)
assert rc != 0 and b"bits 16-27" in lib.pcgc_last_error(), (rc, lib.pcgc_last_error())
print("refused")
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PCGC_DEBUG_SIGNS="1"), capture_output=True, timeout=600)
    assert r.returncode == 0 and b"refused" in r.stdout, r.stderr.decode()[-2000:]
