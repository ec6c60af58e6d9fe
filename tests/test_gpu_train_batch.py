"""-m gpu: the forward and bwd-data kernels of the training step at the launch sizes where their launchers change form, against
the float64 references of tests/_train_batch_ref.py (pinned to the oracle on the CPU by tests/test_train_batch_ref_host.py, which
also proves that the integer rows below are exact in float32 whatever the summation order).  `train_hyper.py --batch_size N` hands
the batch to the library whole; DESIGN.md section 5c lists every branch that depends on it.

(a) the fused C = 32 block at 32^3, pcgc_vrn_fwd_train and pcgc_vrn_fwd_train_signs, at 16 and 17 cubes: launch_vrn32_row_train
    runs vrn32a_row_kernel<1,2,true> / vrn32bc_row_kernel<2,true> up to 16 cubes and <2,4,true> / <8,true> above.  Integer
    operands: every kept tensor and every sign word EQUAL the reference.  Gaussian operands: 2e-5 * max(1, max|ref|), the bound
    tests/test_gpu_train_q4.py::_bound holds these kernels to.  Every slot equals the same cube run alone (the other form at 17
    cubes) bit for bit, and a second run gives the same bits.
(b) pcgc_conv3d_bwd_data_fused at 19 and 20 cubes of the 16^3 stage (launch_conv_mfma: `small` up to 19), five forms of the
    epilogue, and one shape at 32^3 at 2 and 3 cubes.  The float64 reference covers the first, middle and last cube; every slot
    equals that cube in a launch of its own (always the small form) bit for bit.
(c) one whole step on 20 distinct cubes of 64^3 against the mean of its 20 single-cube steps.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _train_batch_ref as R                                  # noqa: E402
from pcgcv1_amd import _lib, synthetic                        # noqa: E402

P = _lib.dptr
NAN = float("nan")


def _bound(ref):
    """tests/test_gpu_train_q4.py::_bound"""
    return 2e-5 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ (a) the fused block forward
_D, _C, _Q = 32, 32, 8
_blocks = {}


def _block_case(B, kind, dev):
    """Operands on the device and their float64 reference, once per (B, kind) and left unchanged."""
    key = (B, kind)
    if key not in _blocks:
        x, params = R.block_operands(kind, B, _D, _C, seed=100 * B + (7 if kind == "int" else 11))
        x, params = x.to(dev), [p.to(dev) for p in params]
        ref = R.block_reference(x, params)
        _blocks[key] = (x, params, ref, R.sign_words(ref.pre))
    return _blocks[key]


def _run_block(entry, x, params):
    """-> (t11, t21, t22, pre or sign words, out); every output pre-filled with what no result equals."""
    lib = _lib.hip()
    B = int(x.shape[0])
    arr = ctypes.cast((ctypes.c_void_p * 10)(*[p.data_ptr() for p in params]), ctypes.c_void_p)
    t = [torch.full((B, _D, _D, _D, _Q), NAN, device=x.device) for _ in range(3)]
    if entry == "signs":
        pre, fn = torch.full((B, _D, _D, _D), 0x2aaaaaaa, dtype=torch.int32, device=x.device), lib.pcgc_vrn_fwd_train_signs
    else:
        pre, fn = torch.full_like(x, NAN), lib.pcgc_vrn_fwd_train
    out = torch.full_like(x, NAN)
    _lib.check(fn(P(x), arr, P(t[0]), P(t[1]), P(t[2]), P(pre), P(out), B, _D, _C, _lib.stream()), "pcgc_vrn_fwd_train" + ("_signs" if entry == "signs" else ""))
    torch.cuda.synchronize()
    return t[0], t[1], t[2], pre, out


@pytest.mark.parametrize("B", [b for b, _, _ in R.BLOCK_CASES])
def test_fused_block_forward_equals_float64_on_integer_operands(B):
    dev = _lib.require_gpu()
    x, params, ref, words = _block_case(B, "int", dev)
    # the exactness condition is one on the operands: their ranges, as test_train_batch_ref_host.py assumes them
    assert float(x.min()) == 0 and float(x.max()) == R.X_MAX and torch.equal(x, x.round())
    for p in params:
        assert float(p.abs().max()) <= (R.BIAS_MAX if p.dim() == 1 else R.W_MAX) and torch.equal(p, p.round())
    assert max(R.block_abs_bound(_C).values()) < R.EXACT
    frac = float((ref.pre > 0).double().mean())
    assert 0.05 < frac < 0.95, frac
    assert not torch.equal(x[0], x[B - 1])
    for entry in ("full", "signs"):
        t11, t21, t22, pre, out = _run_block(entry, x, params)
        for name, got in (("t11", t11), ("t21", t21), ("t22", t22), ("out", out)):
            want = getattr(ref, name)
            bad = got.double() != want                       # NaN (an element never written) differs from everything
            assert not bool(bad.any()), "%s B=%d %s: %d elements differ, first at %s" % (entry, B, name, int(bad.sum()), bad.nonzero()[0].tolist())
        if entry == "signs":
            bad = pre != words
            assert not bool(bad.any()), "signs B=%d: %d sign words differ, first at %s" % (B, int(bad.sum()), bad.nonzero()[0].tolist())
        else:
            bad = pre.double() != ref.pre
            assert not bool(bad.any()), "full B=%d pre: %d elements differ, first at %s" % (B, int(bad.sum()), bad.nonzero()[0].tolist())
    print("block B=%d int: equal to float64 in both entries; %.1f %% of pre positive, largest value %d" % (B, 100 * frac, int(ref.out.max())))


@pytest.mark.parametrize("B", [b for b, _, _ in R.BLOCK_CASES])
def test_fused_block_forward_within_the_float32_bound_on_gaussian_operands(B):
    dev = _lib.require_gpu()
    x, params, ref, _ = _block_case(B, "gauss", dev)
    runs = {}
    for entry in ("full", "signs"):
        t11, t21, t22, pre, out = runs[entry] = _run_block(entry, x, params)
        worst = []
        for name, got in (("t11", t11), ("t21", t21), ("t22", t22), ("out", out)) + ((("pre", pre),) if entry == "full" else ()):
            want = getattr(ref, name)
            assert bool(torch.isfinite(got).all()), (entry, name)
            err, tol = float((got.double() - want).abs().max()), _bound(want)
            worst.append("%s %.3g / %.3g" % (name, err, tol))
            assert err <= tol, (entry, B, name, err, tol)
        print("block B=%d gauss %s: max err / bound  %s" % (B, entry, "; ".join(worst)))
        again = _run_block(entry, x, params)
        for u, v in zip(runs[entry], again):
            assert torch.equal(u, v), (entry, "run to run")
    # the sign words: bit c = (pre[c] > 0) wherever the reference is further from zero than the kernels' bound
    signs, tol = runs["signs"][3], _bound(ref.pre)
    bits = torch.stack([(signs >> c) & 1 for c in range(_C)], dim=-1).bool()
    differ = bits != (ref.pre > 0)
    assert not bool((differ & (ref.pre.abs() > tol)).any())
    assert torch.equal(bits, runs["full"][3] > 0)             # ... and exactly the signs of the `pre` the other entry stores
    print("block B=%d gauss signs: %d of %d bits differ from float64, all within %.3g of zero" % (B, int(differ.sum()), differ.numel(), tol))
    for i in (0, 1, 2, 4):
        assert torch.equal(runs["full"][i], runs["signs"][i]), i


@pytest.mark.parametrize("B", [b for b, _, _ in R.BLOCK_CASES])
def test_fused_block_forward_slots_equal_the_cube_run_alone(B):
    """launch_vrn32_row's comment: the tile forms form "the same sums" — per output bias, then (plane, channel, kh, kw), whatever
    rows x planes a wave walks.  So slot b of a 17-cube launch (2 x 4 / 1 x 8 tiles) must carry the bits of cube b in a launch of
    its own (1 x 2 tiles), in every kept tensor and sign word; at 16 cubes both launches run the same form."""
    dev = _lib.require_gpu()
    x, params, _, _ = _block_case(B, "gauss", dev)
    for entry in ("full", "signs"):
        whole = _run_block(entry, x, params)
        for b in range(B):
            alone = _run_block(entry, x[b:b + 1], params)
            for name, u, v in zip(("t11", "t21", "t22", "pre", "out"), whole, alone):
                assert torch.equal(u[b:b + 1], v), "%s B=%d slot %d: %s differs from the cube run alone" % (entry, B, b, name)


# ------------------------------------------------------------------ (b) bwd-data with the training epilogues
def _bwd_data(layer, ops, form, ws, sl=None):
    """pcgc_conv3d_bwd_data_fused on the cubes sl (a slice of the batch; None: all) -> dx"""
    cin, cout, k, stride, tr, D = layer
    lib = _lib.hip()
    pick = (lambda t: t) if sl is None else (lambda t: t[sl])
    dz, mask, add = pick(ops["dz"]), pick(ops["mask"]), pick(ops["add_to"])
    B = int(dz.shape[0])
    if form == "add_to aliasing dx":
        dx = add.clone()
        add_in, mask_in = dx, None
    else:
        dx = torch.full((B, D, D, D, cin), NAN, device=dz.device)
        add_in, mask_in = (add if "add_to" in form else None), (mask if "mask" in form else None)
    _lib.check(lib.pcgc_conv3d_bwd_data_fused(P(dz), P(ops["w"]), P(dx), P(mask_in), P(add_in), B, D, cin, cout, k, stride, tr, P(ws), ws.numel(),
                                              _lib.stream()), "pcgc_conv3d_bwd_data_fused")
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("case", R.BWD_CASES, ids=R.bwd_case_id)
def test_bwd_data_epilogues_on_either_side_of_the_small_launch_threshold(case):
    dev = _lib.require_gpu()
    layer, B = case
    cin, cout, k, stride, tr, D = layer
    ws = torch.empty(int(_lib.hip().pcgc_conv3d_bwd_workspace_bytes(cin, cout, k)), dtype=torch.uint8, device=dev)
    three = sorted({0, B // 2, B - 1})
    idx = torch.tensor(three, device=dev)
    assert R.adjoint_abs_bound(cout, k) < R.EXACT
    report = []
    for kind in ("int", "gauss"):
        ops = {n: t.to(dev) for n, t in R.bwd_data_operands(kind, layer, B, seed=1000 * R.BWD_CASES.index(case) + (7 if kind == "int" else 11)).items()}
        if kind == "int":
            for n, top in (("dz", R.DZ_MAX), ("w", R.W_MAX), ("add_to", R.ADD_MAX), ("mask", R.X_MAX)):
                assert float(ops[n].abs().max()) <= top and torch.equal(ops[n], ops[n].round()), n
        adj = R.conv_adjoint(ops["dz"][idx].double(), ops["w"].double(), D, stride, bool(tr))       # float64, three cubes, once per kind
        keep, add = (ops["mask"][idx] > 0).double(), ops["add_to"][idx].double()
        assert float(adj.abs().max()) > 0 and 0.2 < float(keep.mean()) < 0.8
        got = {}
        for form in R.BWD_FORMS:
            want = adj + add if "add_to" in form else adj
            want = want * keep if "mask" in form else want
            dx = got[form] = _bwd_data(layer, ops, form, ws)
            assert bool(torch.isfinite(dx).all()), (kind, form)
            if kind == "int":
                bad = dx[idx].double() != want
                assert not bool(bad.any()), "%s %s: %d elements differ from float64, first at %s" % (R.bwd_case_id(case), form, int(bad.sum()), bad.nonzero()[0].tolist())
            else:
                err, tol = float((dx[idx].double() - want).abs().max()), _bound(want)
                report.append("%s %.3g / %.3g" % (form, err, tol))
                assert err <= tol, (R.bwd_case_id(case), form, err, tol)
            # every slot = that cube in a launch of its own
            for b in range(B):
                alone = _bwd_data(layer, ops, form, ws, slice(b, b + 1))
                assert torch.equal(dx[b:b + 1], alone), "%s %s %s: slot %d differs from the cube run alone" % (R.bwd_case_id(case), kind, form, b)
        assert torch.equal(got["add_to"], got["add_to aliasing dx"])                 # in place: each element is read before it is written
        assert torch.equal(_bwd_data(layer, ops, "mask + add_to", ws), got["mask + add_to"])      # run to run
        assert not torch.equal(got["plain"], got["add_to"]) and not torch.equal(got["plain"], got["mask"])
    print("%s (%s launch): int equal in 5 forms; gauss max err / bound  %s" % (R.bwd_case_id(case), "small" if R.is_small_launch(layer, B) else "large", "; ".join(report)))


# ------------------------------------------------------------------ (c) the whole step at 20 cubes
_TERMS = ("loss", "bpp_y", "bpp_z", "empty", "full")
_N = 20


def _symmetries(cube, n):
    """n distinct axis symmetries (permutations and flips) of one [D, D, D, 1] cube, in a fixed order."""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for flips in itertools.product((False, True), repeat=3):
            c = np.transpose(cube, perm + (3,))
            c = np.flip(c, axis=tuple(a for a in range(3) if flips[a])) if any(flips) else c
            out.append(np.ascontiguousarray(c))
    picked = out[::2][:n]                                     # every permutation, four flips of each
    assert len(picked) == n
    for i in range(n):
        for j in range(i):
            assert not np.array_equal(picked[i], picked[j]), (i, j)
    return np.stack(picked)


def _ratios(tr, g, mean):
    """norm(g - mean) / norm(mean), and per parameter tensor max|g - mean| / max|mean| -> (float, {name: float})"""
    d = g.double() - mean
    per, off = {}, 0
    for name, p in tr.p.items():
        n = p.numel()
        top = float(mean[off:off + n].abs().max())
        assert top > 0, name
        per[name] = float(d[off:off + n].abs().max()) / top
        off += n
    assert off == g.numel()
    return float(d.norm()) / float(mean.norm()), per


def test_step_at_20_cubes_is_the_mean_of_its_single_cube_steps():
    """A step at 20 cubes of 64^3 takes every large-launch branch at once: the 32^3 blocks' 2 x 4 / 1 x 8 tiles, the
    16^3 stage's 4 x 4-row conv tiles with the reverse epilogues and the single calls in place of the two-layer launches, the dW
    group counts, the plan's pools, the loss sums with their normalisers formed on the device, and the 8^3 planes-per-wave choice.

    Oracle: the 20 cubes are distinct axis symmetries of one cube, so each holds the same number of occupied (and empty) voxels;
    every loss term divides by the batch's counts, hence each term is the mean of the single-cube terms and the batch gradient the
    mean of the 20 single-cube gradients — and a single-cube step runs the small forms, which test_gpu_train.py anchors to torch
    autograd.  Bound: the same comparison for a batch of TWO (cubes 0 and 1; forms that are anchored as well) measures what float32
    accumulation over a batch costs; the error of a sum of N terms grows like sqrt(N) and sqrt(20 / 2) = 3.2, so 4 times the
    two-cube figure is allowed — for norm(g - mean) / norm(mean), and per parameter tensor for max|g - mean| / max|mean|, where
    the two-cube figure is the worst over the tensors (one tensor's own figure can be exactly zero).  The loss terms: within
    1e-5 * max(1, |mean|), what test_q4_training_layout_gives_the_same_step allows two forms of the same step.  Peak device
    memory: 6 GiB at 8 cubes (test_config4_full_size_step) scaled by 20 / 8 = 15 GiB.
    Measured on an MI355X (profiles/train_batch_tests.txt): two cubes 5.03e-8 (norm) and 2.79e-7 (worst tensor), hence m = 2.01e-7
    and 1.11e-6; twenty cubes 8.53e-8 and 6.49e-7; peak 10.68 GiB."""
    from pcgcv1_amd.train_hyper import Trainer
    _lib.require_gpu()
    w = synthetic.make_weights(seed=29, profile="dense")
    w["hyper_decoder/conv4_2/bias"] = (w["hyper_decoder/conv4_2/bias"] + 0.8).astype(np.float32)      # likelihoods off their floor
    x = _symmetries(synthetic.make_cubes(seed=29, n_cubes=1, cube_size=64)[0], _N)
    assert x.shape == (_N, 64, 64, 64, 1) and len({float(c.sum()) for c in x}) == 1
    rng = np.random.default_rng(29)
    ny = (rng.random((_N, 16, 16, 16, 16)) - 0.5).astype(np.float32)
    nz = (rng.random((_N, 8, 8, 8, 8)) - 0.5).astype(np.float32)
    tr = Trainer(w, alpha=0.75, beta=3.0)

    singles, single_terms = [], []
    for i in range(_N):
        single_terms.append(tr.forward_backward(x[i:i + 1], ny[i:i + 1], nz[i:i + 1]))
        singles.append(tr.flat_g.double())
    assert len({t["num_points"] for t in single_terms}) == 1

    def against_singles(n, what):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        terms = tr.forward_backward(x[:n], ny[:n], nz[:n])
        peak = torch.cuda.max_memory_allocated() - base
        g = tr.flat_g.clone()
        assert bool(torch.isfinite(g).all()) and terms["num_points"] == n * single_terms[0]["num_points"]
        mean = torch.stack(singles[:n]).mean(0)
        for k in _TERMS:
            want = float(np.mean([t[k] for t in single_terms[:n]]))
            print("%s: %s %.9g, mean of the single steps %.9g" % (what, k, terms[k], want))
            assert abs(terms[k] - want) <= 1e-5 * max(1.0, abs(want)), (what, k, terms[k], want)
        assert torch.equal(tr.flat_g, g) and tr.forward_backward(x[:n], ny[:n], nz[:n]) == terms and torch.equal(tr.flat_g, g)      # run to run
        return _ratios(tr, g, mean) + (peak,)

    base_norm, base_per, _ = against_singles(2, "2 cubes")
    base_max = max(base_per.values())
    m_norm, m_max = 4.0 * base_norm, 4.0 * base_max
    norm20, per20, peak = against_singles(_N, "20 cubes")
    worst = sorted(((v, k) for k, v in per20.items()), reverse=True)
    print("2 cubes against the mean of 2 single steps: norm ratio %.4g, worst tensor ratio %.4g (%s)" % (base_norm, base_max, max(base_per, key=base_per.get)))
    print("20 cubes against the mean of 20 single steps: norm ratio %.4g (allowed m = %.4g), worst tensor ratios %s (allowed %.4g)" % (
        norm20, m_norm, ", ".join("%.4g %s" % t for t in worst[:3]), m_max))
    print("peak device memory of the 20-cube step: %.2f GiB" % (peak / 2 ** 30))
    assert base_norm > 0 and base_max > 0
    assert norm20 <= m_norm, (norm20, m_norm)
    for v, name in worst:
        assert v <= m_max, (name, v, m_max)
    assert peak < 15 * 2 ** 30, "20-cube step: peak device memory %.2f GiB" % (peak / 2 ** 30)
