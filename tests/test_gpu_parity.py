"""-m gpu: parity of the HIP path (through the C ABI) against the CPU oracle on seeded inputs."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import entropy as oent            # noqa: E402
from oracle import nets as onets              # noqa: E402
from oracle import points as opoints          # noqa: E402
from oracle import transform as otransform    # noqa: E402
from pcgcv1_amd import _lib, checkpoint, process, synthetic, transform   # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402
from pcgcv1_amd.models import model_voxception as model                  # noqa: E402
from pcgcv1_amd.models.conditional_entropy_model import SymmetricConditional   # noqa: E402
from pcgcv1_amd.models.entropy_model import EntropyBottleneck            # noqa: E402

ATOL = 1e-5          # activations are O(1); the reference's own enc/dec GPU noise is 1.14e-5 (demo.ipynb:780)


def _close(a, b, what, tol=ATOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, "%s: max|diff| %.3g > %.3g" % (what, err, tol * scale)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)


CONV_CASES = [
    # cin, cout, k, stride, transposed, D
    (1, 16, 3, 1, False, 16), (16, 4, 3, 1, False, 16), (4, 8, 3, 1, False, 16), (16, 4, 1, 1, False, 16),
    (4, 4, 3, 1, False, 32), (4, 8, 1, 1, False, 16), (16, 32, 3, 2, False, 32), (32, 8, 3, 1, False, 16),
    (8, 16, 3, 1, False, 16), (8, 8, 3, 1, False, 16), (32, 8, 1, 1, False, 16), (8, 16, 1, 1, False, 16),
    (32, 64, 3, 2, False, 32), (64, 16, 3, 1, False, 16), (16, 32, 3, 1, False, 16), (64, 16, 1, 1, False, 16),
    (16, 16, 3, 1, False, 16), (16, 32, 1, 1, False, 16), (16, 64, 3, 1, False, 16), (64, 32, 3, 2, True, 16),
    (32, 16, 3, 2, True, 16), (16, 1, 3, 1, False, 16), (16, 16, 3, 2, False, 16), (16, 8, 3, 1, False, 8),
    (8, 16, 3, 1, False, 8), (16, 16, 3, 2, True, 8), (32, 16, 3, 1, False, 16), (16, 16, 3, 2, True, 16),
    # model_simple.py:20-41, 56-86: 9^3 and 5^3, stride 2 and transposed
    (1, 32, 9, 2, False, 16), (32, 32, 5, 2, False, 16), (32, 32, 5, 2, True, 8), (32, 1, 9, 2, True, 8), (4, 4, 5, 1, False, 8),
]


@pytest.mark.parametrize("cin,cout,k,stride,transposed,D", CONV_CASES)
def test_conv_layer_vs_oracle(cin, cout, k, stride, transposed, D):
    rng = np.random.default_rng(cin * 1000 + cout * 10 + k + D)
    B = 2
    x = rng.standard_normal((B, D, D, D, cin)).astype(np.float32)
    kshape = (k, k, k, cout, cin) if transposed else (k, k, k, cin, cout)
    w = (rng.standard_normal(kshape) / np.sqrt(k ** 3 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ref = onets.conv3d_transpose_same(x, w, b, relu=True) if transposed else onets.conv3d_same(x, w, b, stride=stride, relu=True)
    xd, wd, bd = (torch.from_numpy(a).cuda() for a in (x, w, b))
    direct = model.conv3d(xd, wd, bd, stride=stride, transposed=transposed, relu=True, algo=1).cpu().numpy()
    _close(direct, ref, "direct kernel")
    auto = model.conv3d(xd, wd, bd, stride=stride, transposed=transposed, relu=True, algo=0).cpu().numpy()
    _close(auto, ref, "auto (MFMA where available) kernel")
    nobias = model.conv3d(xd, wd, None, stride=stride, transposed=transposed, relu=False, algo=0).cpu().numpy()
    ref2 = onets.conv3d_transpose_same(x, w, None) if transposed else onets.conv3d_same(x, w, None, stride=stride)
    _close(nobias, ref2, "no-bias linear")


def test_mfma_layout_is_transpose_safe():
    """Asymmetric weights and inputs (A=I-style check): a swapped row/col mapping cannot pass."""
    D, cin, cout = 16, 16, 16
    x = np.zeros((1, D, D, D, cin), np.float32)
    x[0, 5, 6, 7, 3] = 1.0
    w = np.zeros((3, 3, 3, cin, cout), np.float32)
    w[0, 1, 2, 3, 11] = 2.0          # one tap, one (ci, co) pair
    y = model.conv3d(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), None, algo=2).cpu().numpy()
    nz = np.argwhere(y != 0)
    assert nz.tolist() == [[0, 5 + 1 - 0, 6 + 1 - 1, 7 + 1 - 2, 11]] and y[tuple(nz[0])] == 2.0


@pytest.mark.parametrize("C,D,B", [(16, 64, 2), (16, 64, 1), (32, 32, 3), (64, 16, 5), (32, 16, 2), (16, 16, 1)])
def test_vrn_block_vs_oracle(C, D, B):
    """pcgc_vrn_fwd: C=16 at D=64 is the v_mfma_f32_4x4x1 row-kernel pair of the transforms' full-resolution stage
    (incl. the cube faces, where rows / planes / lanes outside the cube must read as zeros)."""
    rng = np.random.default_rng(C * 100 + D + B)
    q, h = C // 4, C // 2
    shapes = {"conv1_1": (3, C, q), "conv1_2": (3, q, h), "conv2_1": (1, C, q), "conv2_2": (3, q, q), "conv2_3": (1, q, h)}
    w, params = {}, []
    for name in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv2_3"):
        k, ci, co = shapes[name]
        w["b/%s/kernel" % name] = (rng.standard_normal((k, k, k, ci, co)) * np.sqrt(2.0 / (k ** 3 * ci))).astype(np.float32)
        w["b/%s/bias" % name] = (rng.standard_normal(co) * 0.1).astype(np.float32)
        params += [torch.from_numpy(w["b/%s/kernel" % name]).cuda(), torch.from_numpy(w["b/%s/bias" % name]).cuda()]
    x = np.maximum(rng.standard_normal((B, D, D, D, C)), 0).astype(np.float32)
    x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = 1.5, -0.5, 2.0, 0.25, 1.0, 3.0   # faces
    ref = onets.vrn_block(w, "b", x)
    xd = torch.from_numpy(x).cuda()
    y = model.vrn_block(xd, params)
    _close(y.cpu().numpy(), ref, "vrn block C=%d D=%d" % (C, D))
    assert torch.equal(model.vrn_block(xd, params), y)                        # run to run
    if B > 1:
        assert torch.equal(model.vrn_block(xd[1:2].contiguous(), params), y[1:2])   # batch-slot invariant


def test_vrn_block_full_launch_is_slot_invariant():
    """Eight copies of one cube = one full row-kernel launch (2048 waves, two per SIMD): every copy's output equals the
    first and a second run equals the first bit for bit.  Regression for a store-data hazard that only shows when two
    waves share a SIMD (a 128-bit buffer store with a register soffset, its data register rewritten by the next VALU
    instruction: cubes 4..7 of the launch came out different from run to run)."""
    rng = np.random.default_rng(5)
    C, D, B = 16, 64, 8
    q, h = C // 4, C // 2
    shapes = {"conv1_1": (3, C, q), "conv1_2": (3, q, h), "conv2_1": (1, C, q), "conv2_2": (3, q, q), "conv2_3": (1, q, h)}
    params = []
    for name in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv2_3"):
        k, ci, co = shapes[name]
        params += [torch.from_numpy((rng.standard_normal((k, k, k, ci, co)) * np.sqrt(2.0 / (k ** 3 * ci))).astype(np.float32)).cuda(),
                   torch.from_numpy((rng.standard_normal(co) * 0.1).astype(np.float32)).cuda()]
    x1 = torch.from_numpy(np.maximum(rng.standard_normal((1, D, D, D, C)), 0).astype(np.float32)).cuda()
    x = x1.expand(B, D, D, D, C).contiguous()
    y = model.vrn_block(x, params)
    for b in range(1, B):
        assert torch.equal(y[b], y[0]), "cube %d of the launch differs from cube 0" % b
    for _ in range(3):
        assert torch.equal(model.vrn_block(x, params), y)


@pytest.mark.parametrize("n_cubes", [64, 9])
def test_every_row_kernel_is_slot_invariant_and_repeatable(n_cubes):
    """The register-allocation conventions the row kernels rely on (csrc/row_common.h mfa_new, csrc/vrn_row.hip rsrc_at; the
    object code is checked by tools/check_isa.py) guard against a hazard that showed only with two waves per SIMD and only
    in some slots of a launch, differently from run to run.  So: identical cubes in EVERY slot of full launches through all
    four networks — every row kernel of the inference path (64^3: conv_in, VRN A / BC, down_1, up_2, deconv_out; 32^3:
    VRN A / BC, down_2, up_1; 16^3: VRN A / B / C and the 16x16x4 layers; 8^3 hyper layers) at its real occupancy — every
    slot's result must equal slot 0's, and five repetitions must equal the first, bit for bit.  n_cubes = 9 adds the
    partially filled last launch and the small-launch tile variants."""
    checkpoint._CACHE["t_slots"] = synthetic.make_weights(seed=23, profile="dense")
    c = transform.get_codec(model, "t_slots")
    x1 = torch.from_numpy(synthetic.make_cubes(seed=23, n_cubes=1)).cuda()
    x = x1.expand(n_cubes, 64, 64, 64, 1).contiguous()

    def run():
        y = c.analysis_transform(x)
        z = c.hyper_encoder(y)
        z_hat, _ = c.entropy_bottleneck(z, False)
        loc, scale = c.hyper_decoder(z_hat, lower_bound=1e-9)
        xs = c.synthesis_transform(torch.round(y))
        return y, z, loc, scale, xs
    first = run()
    for name, t in zip(("analysis", "hyper_encoder", "loc", "scale", "synthesis"), first):
        for b in range(1, n_cubes):
            assert torch.equal(t[b], t[0]), "%s: slot %d of %d differs from slot 0" % (name, b, n_cubes)
    for rep in range(5):
        again = run()
        for name, a, b in zip(("analysis", "hyper_encoder", "loc", "scale", "synthesis"), again, first):
            assert torch.equal(a, b), "%s: repetition %d differs from the first run" % (name, rep + 1)


@pytest.mark.parametrize("n_cubes", [79, 39, 24])
def test_tiles_chosen_by_launch_size_do_not_change_a_bit(n_cubes, monkeypatch):
    """The 32^3 / 16^3 block kernels and down_2 pick their wave tile by launch size (a chunk's remainder must not run as a
    ragged round of the full chunk's tiles: profiles/r05_vH_tile_by_launch_size.txt).  The sums per output do not depend on the
    tile: every forced tile (PCGC_A32_TILE, PCGC_BC32_LD, PCGC_DOWN2_LD, PCGC_V64_LD; read per launch) gives the bits of the
    default choice, for launch sizes on both sides of every threshold — the decoder's slices (24, 79) and a 32^3 remainder (39)."""
    import os
    checkpoint._CACHE["t_tiles"] = synthetic.make_weights(seed=29, profile="dense")
    c = transform.get_codec(model, "t_tiles")
    x = torch.from_numpy(synthetic.make_cubes(seed=29, n_cubes=8)).cuda()
    x = x.repeat((n_cubes + 7) // 8, 1, 1, 1, 1)[:n_cubes].contiguous()

    def run():
        y = c.analysis_transform(x)
        return y, c.synthesis_transform(torch.round(y))
    y0, s0 = run()
    assert float(y0.abs().max()) > 0 and float(s0.abs().max()) > 0
    for env in ({"PCGC_A32_TILE": "24", "PCGC_BC32_LD": "8", "PCGC_DOWN2_LD": "2", "PCGC_V64_LD": "0"},     # the fixed tiles of round 4
                {"PCGC_A32_TILE": "28", "PCGC_BC32_LD": "16", "PCGC_DOWN2_LD": "4", "PCGC_V64_LD": "4"},
                {"PCGC_A32_TILE": "14", "PCGC_BC32_LD": "4", "PCGC_DOWN2_LD": "1", "PCGC_V64_LD": "1"},
                {"PCGC_V64_LD": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        y1, s1 = run()
        for k in env:
            monkeypatch.delenv(k)
        assert torch.equal(y1, y0), ("analysis", env)
        assert torch.equal(s1, s0), ("synthesis", env)


@pytest.mark.parametrize("n_cubes", [1, 5, 19])
def test_small_launch_forms_do_not_change_a_bit(n_cubes, monkeypatch):
    """Below 20 cubes the 16^3 stage's layers (stride 1, down_2, up_1) run as SMALL launches: 2 x 2-row tiles, software-pipelined
    (conv_mfma_small_body, tconv_mfma_small_kernel).  Against the same tiles on conv_mfma_body (PCGC_CONV_PIPE=0) and against
    the large launches' 4 x 4-row tiles (PCGC_SMALL_TILES=0), both read per launch: the same sums per output, so the same
    latents and the same logits bit for bit — analysis (with empty-space skipping) and synthesis."""
    checkpoint._CACHE["t_small"] = synthetic.make_weights(seed=31, profile="dense")
    c = transform.get_codec(model, "t_small")
    x = torch.from_numpy(synthetic.make_cubes(seed=31, n_cubes=8)).cuda()
    x = x.repeat((n_cubes + 7) // 8, 1, 1, 1, 1)[:n_cubes].contiguous()

    def run():
        y = c.analysis_transform(x)
        return y, c.synthesis_transform(torch.round(y))
    y0, s0 = run()
    assert float(y0.abs().max()) > 0 and float(s0.abs().max()) > 0
    for env in ({"PCGC_CONV_PIPE": "0"}, {"PCGC_SMALL_TILES": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        y1, s1 = run()
        for k in env:
            monkeypatch.delenv(k)
        assert torch.equal(y1, y0), ("analysis", env)
        assert torch.equal(s1, s0), ("synthesis", env)


@pytest.fixture(scope="module")
def dense():
    w = synthetic.make_weights(seed=11, profile="dense")
    checkpoint._CACHE["t_dense"] = w
    return w


def test_transforms_vs_oracle_and_direct(dense):
    x = synthetic.make_cubes(seed=3, n_cubes=2)
    c = transform.get_codec(model, "t_dense")
    xd = torch.from_numpy(x).cuda()
    y_ref = onets.analysis_transform(onets.sub(dense, "analysis_transform"), x)
    y = c.analysis_transform(xd)
    _close(y.cpu().numpy(), y_ref, "analysis (MFMA path)", 2e-5)
    y_dir = c.analysis_transform.set_algo(1)(xd)
    c.analysis_transform.set_algo(0)
    _close(y_dir.cpu().numpy(), y_ref, "analysis (direct path)", 2e-5)
    z_ref = onets.hyper_encoder(onets.sub(dense, "hyper_encoder"), y_ref)
    _close(c.hyper_encoder(torch.from_numpy(y_ref).cuda()).cpu().numpy(), z_ref, "hyper encoder")
    zq = np.rint(z_ref)
    loc_ref, scale_ref = onets.hyper_decoder(onets.sub(dense, "hyper_decoder"), zq)
    loc, scale = c.hyper_decoder(torch.from_numpy(zq).cuda(), lower_bound=1e-9)
    _close(loc.cpu().numpy(), loc_ref, "hyper decoder loc")
    _close(scale.cpu().numpy(), np.maximum(scale_ref, 1e-9), "hyper decoder scale")
    yq = np.rint(y_ref)
    x_ref = onets.synthesis_transform(onets.sub(dense, "synthesis_transform"), yq)
    xt = c.synthesis_transform(torch.from_numpy(yq).cuda())
    _close(xt.cpu().numpy(), x_ref, "synthesis (MFMA path)", 2e-5)


def test_results_do_not_depend_on_batch_slot_or_size(dense):
    """The decoder must regenerate the encoder's loc/scale bit for bit (README.md:111-114)."""
    c = transform.get_codec(model, "t_dense")
    rng = np.random.default_rng(5)
    z = torch.from_numpy(np.rint(rng.standard_normal((7, 8, 8, 8, 8)) * 2).astype(np.float32)).cuda()
    loc7, sc7 = c.hyper_decoder(z, lower_bound=1e-9)
    loc1, sc1 = c.hyper_decoder(z[4:5].contiguous(), lower_bound=1e-9)
    assert torch.equal(loc7[4:5], loc1) and torch.equal(sc7[4:5], sc1)
    y = torch.from_numpy(np.rint(rng.standard_normal((5, 16, 16, 16, 16)) * 2).astype(np.float32)).cuda()
    a = c.synthesis_transform(y)
    b = c.synthesis_transform(y[3:4].contiguous())
    assert torch.equal(a[3:4], b)
    assert torch.equal(c.synthesis_transform(y), a)              # run-to-run


def test_entropy_models_vs_oracle(dense):
    rng = np.random.default_rng(8)
    y = (rng.standard_normal((2, 16, 16, 16, 16)) * 2).astype(np.float32)
    y[0, 0, 0, 0, :4] = [0.5, 1.5, -0.5, 2.5]                     # round-half-even cases
    loc = (rng.standard_normal(y.shape) * 0.7).astype(np.float32)
    scale = np.maximum(np.abs(rng.standard_normal(y.shape)) * 0.8, 1e-9).astype(np.float32)
    loc[0, 0, 0, 1, 0], y[0, 0, 0, 1, 0] = 2.0, 1.0              # sign(2q - loc) == 0 quirk
    sc = SymmetricConditional()
    v, lik = sc(y, loc, scale, False)
    v_ref, lik_ref = oent.sc_call(y, loc, scale)
    bits = lambda a: (a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)                      # noqa: E731
    assert np.array_equal(v.cpu().numpy(), v_ref)
    # likelihoods: the oracle's bits, as the pmf of the same function already had to be (measured before it was demanded:
    # 0 of 2 097 925 differ with noise, test_gpu_entropy_forms.py)
    assert np.array_equal(bits(lik), bits(lik_ref))
    assert lik.cpu().numpy()[0, 0, 0, 1, 0] == np.float32(1e-9)
    noise = (rng.random(y.shape) - 0.5).astype(np.float32)
    v, lik = sc(y, loc, scale, True, noise=torch.from_numpy(noise))
    v_ref, lik_ref = oent.sc_call(y, loc, scale, training=True, noise=noise)
    np.testing.assert_allclose(v.cpu().numpy(), v_ref, rtol=0, atol=0)
    assert np.array_equal(bits(lik), bits(lik_ref))
    # factorized prior
    eb = EntropyBottleneck().load_weights(dense, "estimator")
    z = (rng.standard_normal((3, 8, 8, 8, 8)) * 2).astype(np.float32)
    zv, zl = eb(z, False)
    zv_ref, zl_ref = oent.eb_call(onets.sub(dense, "estimator"), z)
    assert np.array_equal(zv.cpu().numpy(), zv_ref)
    assert np.array_equal(bits(zl), bits(zl_ref))
    s, mn, mx = eb.compress(z)
    assert (mn, mx) == (int(np.rint(z).min()), int(np.rint(z).max()))
    assert np.array_equal(eb.decompress(s, mn, mx, z.shape).cpu().numpy(), np.rint(z))
    s_ref, _, _ = oent.eb_compress(onets.sub(dense, "estimator"), z)
    assert bytes(s) == bytes(s_ref)                             # reproducible pmf (repro_math.h): identical strings


def test_symbol_casts_of_the_coder_boundary():
    """The casts either side of the range coder (entropy_model.py:253-258, 298-304; conditional_entropy_model.py:195-199) as the
    kernels that replace them: round-half-even straight to int16 with the range, and decoded int16 symbols + min_v back to
    float32 — against numpy, bit for bit, incl. x.5 ties, -0.0 and a ragged length."""
    from pcgcv1_amd import _lib
    lib, dev = _lib.hip(), _lib.require_gpu()
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(3 * 4096 + 0) * 3).astype(np.float32)
    x[:6] = [0.5, 1.5, -0.5, 2.5, -0.0, -2.5]
    xd = torch.from_numpy(x).to(dev)
    q = torch.empty(x.size, dtype=torch.int16, device=dev)
    mm = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(lib.pcgc_round_minmax_i16(_lib.dptr(xd), _lib.dptr(q), _lib.dptr(mm[0:1]), _lib.dptr(mm[1:2]), x.size, x.size, _lib.stream()))
    want = np.rint(x)
    assert np.array_equal(q.cpu().numpy(), want.astype(np.int16)) and tuple(mm.cpu().numpy()) == (int(want.min()), int(want.max()))
    eb = EntropyBottleneck()
    out = torch.full((x.size,), 9.0, device=dev)
    assert np.array_equal(eb.quantize_into(xd, out).cpu().numpy(), want)
    sym = rng.integers(0, 12, 5 * 777, dtype=np.int16)
    sd = torch.from_numpy(sym).to(dev)
    v = torch.empty(sym.size, dtype=torch.float32, device=dev)
    _lib.check(lib.pcgc_symbols_to_values(_lib.dptr(sd), -7, _lib.dptr(v), sym.size, _lib.stream()))
    assert np.array_equal(v.cpu().numpy(), (sym.astype(np.int32) - 7).astype(np.float32))
    offs = np.array([-3, 0, -15, 2, -1], np.float32)
    _lib.check(lib.pcgc_symbols_to_values_seg(_lib.dptr(sd), _lib.dptr(torch.from_numpy(offs).to(dev)), _lib.dptr(v), sym.size, 777, _lib.stream()))
    assert np.array_equal(v.cpu().numpy(), (sym.reshape(5, 777).astype(np.float32) + offs[:, None]).reshape(-1))


def test_laplace_cdf_rows_vs_oracle():
    """Integer CDF rows produced on the device == the oracle's, every row, bit for bit: the float pmf is built from
    the reproducible exp of repro_math.h on both sides (conditional_entropy_model.py:95-124 + pmf_to_quantized_cdf)."""
    rng = np.random.default_rng(12)
    rows = 4096 * 4
    loc = (rng.standard_normal(rows) * 1.5).astype(np.float32)
    scale = np.maximum(np.abs(rng.standard_normal(rows)) * 1.2, 1e-9).astype(np.float32)
    scale[:8] = [1e-9, 1e-3, 0.05, 0.3, 5.0, 40.0, 0.7, 2.0]
    mn, mx = np.array([-6, -1], np.int32), np.array([7, 1], np.int32)
    seg = rows // 2
    dev = torch.device("cuda")
    cdf = torch.empty((rows, 14), dtype=torch.int16, device=dev)
    lib = _lib.hip()
    args = [torch.from_numpy(a).to(dev) for a in (loc, scale, mn, mx)]
    _lib.check(lib.pcgc_laplace_cdf(_lib.dptr(args[0]), _lib.dptr(args[1]), _lib.dptr(args[2]), _lib.dptr(args[3]), rows,
                                    seg, 14, 1e-9, None, _lib.dptr(cdf), None, _lib.stream()))
    got = cdf.cpu().numpy().view(np.uint16).astype(np.int64)
    for s in range(2):
        n = mx[s] - mn[s] + 1
        sl = slice(s * seg, (s + 1) * seg)
        ref = oent.sc_get_cdf(loc[sl, None], scale[sl, None], int(mn[s]), int(mx[s]))[:, 0, :]     # [seg, n+1]
        assert np.array_equal(got[sl, :n], ref[:, :n]), "%d of %d rows differ" % (int((got[sl, :n] != ref[:, :n]).any(1).sum()), seg)
    # the likelihoods themselves (same function evaluated per element)
    y = np.rint(rng.standard_normal(rows) * 3).astype(np.float32)
    yd, lik = torch.from_numpy(y).to(dev), torch.empty(rows, dtype=torch.float32, device=dev)
    _lib.check(lib.pcgc_laplace_likelihood(_lib.dptr(yd), _lib.dptr(args[0]), _lib.dptr(args[1]), None, None, _lib.dptr(lik), rows,
                                           1e-9, _lib.stream()))
    _, lik_ref = oent.sc_call(y, loc, scale)
    assert np.array_equal(lik.cpu().numpy().view(np.uint32), lik_ref.view(np.uint32))


def test_streams_cross_decode_with_the_oracle(dense):
    """The oracle range-decodes what the HIP path encoded and the HIP path decodes what the oracle encoded — y (one
    Laplace stream per cube) and z (one factorized stream per batch) of C2-like 64^3 cubes, from the loc / scale / z
    the HIP transforms produced.  Every string is also byte-identical between the two implementations."""
    x = synthetic.make_cubes(seed=9, n_cubes=3)
    c = transform.get_codec(model, "t_dense")
    ys = c.analysis_transform(torch.from_numpy(x).cuda())
    zs = c.hyper_encoder(ys)
    # ---- z: factorized prior, one string for the batch (entropy_model.py:223-306)
    est = onets.sub(dense, "estimator")
    z_np = zs.cpu().numpy()
    s_hip, mn, mx = c.entropy_bottleneck.compress(zs)
    s_ref, mn_r, mx_r = oent.eb_compress(est, z_np)
    assert (mn, mx) == (mn_r, mx_r) and bytes(s_hip) == bytes(s_ref)
    pmf_hip = c.entropy_bottleneck._pmf(mn, mx)
    assert np.array_equal(pmf_hip.view(np.uint32), oent.eb_pmf(est, mn, mx).view(np.uint32))
    assert np.array_equal(oent.eb_decompress(est, s_hip, mn, mx, z_np.shape), np.rint(z_np))          # oracle decodes HIP
    z_hat = c.entropy_bottleneck.decompress(s_ref, mn_r, mx_r, z_np.shape)                            # HIP decodes oracle
    assert torch.equal(z_hat, torch.round(zs))
    # ---- y: Laplace prior conditioned on the hyper-decoder output, one string per cube
    loc, scale = c.hyper_decoder(z_hat, lower_bound=1e-9)
    sc = c.conditional_entropy_model
    strings, mns, mxs = sc.compress_cubes(ys, loc, scale)
    y_np, loc_np, scale_np = ys.cpu().numpy(), loc.cpu().numpy(), scale.cpu().numpy()
    oracle_strings = []
    for b in range(3):
        s_o, mn_o, mx_o = oent.sc_compress(y_np[b:b + 1], loc_np[b:b + 1], scale_np[b:b + 1])
        assert (mn_o, mx_o) == (int(mns[b]), int(mxs[b]))
        assert bytes(s_o) == bytes(strings[b]), "cube %d: HIP and oracle strings differ" % b
        oracle_strings.append(s_o)
        dec = oent.sc_decompress(strings[b], loc_np[b:b + 1], scale_np[b:b + 1], mn_o, mx_o, y_np[b:b + 1].shape)
        assert np.array_equal(dec, np.rint(y_np[b:b + 1]))                                            # oracle decodes HIP
    y_dec = sc.decompress_cubes(oracle_strings, loc, scale, mns, mxs, [1, 16, 16, 16, 16])             # HIP decodes oracle
    assert torch.equal(y_dec, torch.round(ys))


def test_laplace_cdf_integer_algorithm_bit_exact():
    """The device quantiser (run-length form of TF's greedy correction) against the oracle's step-by-step C
    restatement on the SAME float pmf: the pmf of every symbol is produced by pcgc_laplace_likelihood (the same
    device function the CDF kernel evaluates), so every row must match exactly — including rows whose support
    holds little of the mass (deficits of tens of thousands) and rows that overshoot (sum > 2^16).
    One launch at ncols = 31, cdf_lower only: that is laplace_cdf_kernel<32> (test_laplace_cdf_rows_vs_oracle, ncols = 14, runs
    <16>).  The instantiations <4> and <8>, which the committed checkpoints run, every ncols at which the choice changes and
    the encoder's lohi output are pinned in test_gpu_entropy_forms.py."""
    from oracle import coder as ocoder
    rng = np.random.default_rng(77)
    rows = 4096 * 6
    loc = (rng.standard_normal(rows) * 2.0).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(60.0), rows)).astype(np.float32)
    scale[:6] = [1e-9, 1e-4, 0.3, 7.0, 100.0, 1e4]
    loc[6:12] = [0.0, 0.5, -0.5, 1.0, 2.0, -3.0]                     # symmetric cases -> exactly tied keys
    scale[6:12] = [0.7, 0.7, 1.3, 0.2, 2.0, 0.9]
    # every segment: exactly symmetric rows (identical key sequences of the two tails: ties at every step), nearly
    # symmetric ones (leaders alternate), and heavy-tailed ones whose support holds little mass (deficits of thousands)
    for s0 in (0, rows // 3, 2 * (rows // 3)):
        k = 512
        loc[s0 + 16:s0 + 16 + k] = 0.0
        loc[s0 + 16 + k:s0 + 16 + 2 * k] = rng.choice([0.5, -0.5, 1.0, -1.0, 1e-4, -3e-5, 0.013, 0.03], k)
        scale[s0 + 16:s0 + 16 + 2 * k] = np.exp(rng.uniform(np.log(0.05), np.log(30.0), 2 * k))
        loc[s0 + 16 + 2 * k:s0 + 16 + 3 * k] = rng.uniform(-0.05, 0.05, k)
        scale[s0 + 16 + 2 * k:s0 + 16 + 3 * k] = rng.uniform(0.1, 0.2, k)     # the bench operating point's heavy rows
    seg = rows // 3
    mn, mx = np.array([-1, -7, -15], np.int32), np.array([1, 8, 15], np.int32)
    dev = torch.device("cuda")
    lib = _lib.hip()
    loc_d, scale_d, mn_d, mx_d = (torch.from_numpy(a).to(dev) for a in (loc, scale, mn, mx))
    ncols = 31
    cdf = torch.empty((rows, ncols), dtype=torch.int16, device=dev)
    _lib.check(lib.pcgc_laplace_cdf(_lib.dptr(loc_d), _lib.dptr(scale_d), _lib.dptr(mn_d), _lib.dptr(mx_d), rows, seg, ncols,
                                    1e-9, None, _lib.dptr(cdf), None, _lib.stream()))
    got = cdf.cpu().numpy().view(np.uint16).astype(np.int64)
    for s in range(3):
        n = int(mx[s] - mn[s] + 1)
        sl = slice(s * seg, (s + 1) * seg)
        pmf = np.empty((seg, n), np.float32)
        for k in range(n):
            yk = torch.full((seg,), float(mn[s] + k), dtype=torch.float32, device=dev)
            lik = torch.empty_like(yk)
            _lib.check(lib.pcgc_laplace_likelihood(_lib.dptr(yk), _lib.dptr(loc_d[sl].contiguous()), _lib.dptr(scale_d[sl].contiguous()),
                                                   None, None, _lib.dptr(lik), seg, 1e-9, _lib.stream()))
            pmf[:, k] = lik.cpu().numpy()
        ref = ocoder.pmf_to_quantized_cdf(pmf)
        assert np.array_equal(got[sl, :n], ref[:, :n]), "segment %d: %d rows differ" % (s, int((got[sl, :n] != ref[:, :n]).any(1).sum()))
        deficit = 65536 - np.maximum(1, np.rint(pmf.astype(np.float32) * np.float32(65536))).sum(1)
        assert deficit.max() > 1000 and deficit.min() < 0          # both branches and long runs were exercised


def test_hyper_codec_roundtrip_and_rate_vs_oracle(dense):
    x = synthetic.make_cubes(seed=4, n_cubes=3)
    out = transform.compress_hyper(x, model, "t_dense", decompress=True)
    y_strings, y_min_vs, y_max_vs, y_shape, z_string, z_min_v, z_max_v, z_shape, x_enc = out
    assert list(y_shape) == [1, 16, 16, 16, 16] and list(z_shape) == [3, 8, 8, 8, 8]
    xs = transform.decompress_hyper(*out[:8], model, "t_dense")
    assert torch.equal(xs, x_enc)                     # decoder == encoder-side reconstruction, bitwise
    # symbols survive the range coder exactly
    c = transform.get_codec(model, "t_dense")
    ys = c.analysis_transform(torch.from_numpy(x).cuda())
    zs = c.hyper_encoder(ys)
    z_dec = c.entropy_bottleneck.decompress(z_string, z_min_v, z_max_v, z_shape)
    assert torch.equal(z_dec, torch.round(zs))
    loc, scale = c.hyper_decoder(z_dec, lower_bound=1e-9)
    y_dec = c.conditional_entropy_model.decompress_cubes(y_strings, loc, scale, y_min_vs, y_max_vs, y_shape)
    assert torch.equal(y_dec, torch.round(ys))
    # rate against the CPU oracle pipeline (same weights, same cubes): strings agree within 1e-3 bpp
    ref = otransform.compress_hyper(x, dense)
    n_pts = float(x.sum())
    bpp = 8.0 * (sum(map(len, y_strings)) + len(z_string)) / n_pts
    bpp_ref = 8.0 * (sum(map(len, ref[0])) + len(ref[4])) / n_pts
    assert abs(bpp - bpp_ref) <= 1e-3 * max(1.0, bpp_ref), (bpp, bpp_ref)
    assert np.array_equal(y_min_vs, ref[1]) and np.array_equal(y_max_vs, ref[2])
    # reconstruction logits against the oracle synthesis fed with OUR decoded symbols (the two conv stacks sum in
    # different orders, so their loc / scale differ in the last bits; cross-decoding on identical loc / scale is
    # test_streams_cross_decode_with_the_oracle)
    x_ref = onets.synthesis_transform(onets.sub(dense, "synthesis_transform"), y_dec.cpu().numpy())
    _close(xs.cpu().numpy(), x_ref, "decoded logits", 5e-5)


def test_topk_and_postprocess_vs_reference_golden(golden):
    g = golden("select.npz")
    vols, nums = g["vols"], g["nums"]
    for rho in (1.0, 1.1, 0.5):
        m = iop.select_voxels(vols, nums, rho).cpu().numpy()
        assert np.array_equal(m, g["mask_rho%g" % rho])
    assert np.array_equal(iop.select_voxels(vols, nums, 1.0, fixed_thres=0.0).cpu().numpy(), g["mask_fixed0"])
    mask = iop.select_voxels(vols, nums, 1.0)
    pts = iop.voxels2points(mask)
    assert [len(p) for p in pts] == list(g["v2p_lens"]) and np.array_equal(np.concatenate(pts), g["v2p_flat"])
    merged = iop.merge_points(pts, g["merge_positions"], 16)
    assert iop.ply_bytes(merged) == g["merge_ply"].tobytes()
    # full-size cube: threshold equals numpy's k-th largest
    rng = np.random.default_rng(2)
    big = (rng.standard_normal((2, 64, 64, 64, 1)) * 4).astype(np.float32)
    k = np.array([4246, 11450])
    ref = opoints.select_voxels(big, k, 1.0)
    assert np.array_equal(iop.select_voxels(big, k, 1.0).cpu().numpy(), ref.astype(np.uint8))


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_preprocess_postprocess_vs_reference_golden(golden, name):
    g = golden("partition.npz")
    cube, min_num, scale = g[name + "_args"]
    cubes, pos, nums = process.preprocess_points(g[name + "_points"], float(scale), int(cube), int(min_num))
    assert np.array_equal(pos, g[name + "_cube_positions"]) and np.array_equal(nums, g[name + "_points_numbers"])
    occ = np.split(g[name + "_occ_flat"], np.cumsum(g[name + "_occ_lens"])[:-1])
    cn = cubes.cpu().numpy()
    for c, o in zip(cn, occ):
        assert np.array_equal(np.flatnonzero(c), o)
    rec = process.postprocess_points(cubes, nums, pos, float(scale), int(cube), 1.0)
    assert iop.ply_bytes(rec) == g[name + "_rec_ply"].tobytes()


def test_block_preprocess_with_negative_coordinates_matches_the_host_voxeliser():
    """pcgc_voxelize_points (device, mod and block filter in the kernel) against the host path that builds the
    per-point records with numpy; negative coordinates take numpy's non-negative remainder."""
    rng = np.random.default_rng(11)
    pts = np.unique(rng.integers(-96, 160, size=(60000, 3)).astype(np.int32), axis=0)
    full, pos, nums = process.preprocess_points(pts, 1.0, 64, 20)
    ref, pos_h, nums_h = process.preprocess_points(pts, 1.0, 64, 20, device=False)
    assert np.array_equal(pos, pos_h) and np.array_equal(nums, nums_h) and int(nums.sum()) > 0
    assert np.array_equal(full.cpu().numpy(), ref)
    got = []
    for r in range(3):
        blk, pos_r, nums_r = process.preprocess_points(pts, 1.0, 64, 20, block=(r, 3))
        assert np.array_equal(pos_r, pos)
        got.append(blk.cpu().numpy())
    assert np.array_equal(np.concatenate(got), ref)


def test_bce_sums_vs_oracle():
    rng = np.random.default_rng(3)
    pred = (rng.standard_normal((2, 32, 32, 32, 1)) * 4).astype(np.float32)
    label = (rng.random(pred.shape) > 0.97).astype(np.float32)
    dev = torch.device("cuda")
    lib = _lib.hip()
    ws = torch.empty(lib.pcgc_bce_workspace_bytes(pred.size), dtype=torch.uint8, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    p, l = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
    _lib.check(lib.pcgc_bce_sums(_lib.dptr(p), _lib.dptr(l), pred.size, _lib.dptr(sums), _lib.dptr(ws), ws.numel(), _lib.stream()))
    s = sums.cpu().numpy()
    e_ref, f_ref = otransform.bce_loss(pred, label)
    assert s[1] + s[3] == pred.size
    assert abs(s[0] / s[1] - e_ref) < 1e-5 * e_ref and abs(s[2] / s[3] - f_ref) < 1e-5 * f_ref


def test_d1_metric_vs_pc_error_golden(golden):
    """pcgc_d1_mse against the numbers MPEG pc_error_d (the reference's myutils binary) printed for seeded clouds."""
    from pcgcv1_amd import metrics
    g = golden("pc_error_d1.npz")
    for i in (0, 1):
        m = metrics.d1_metrics(g["a%d" % i], g["b%d" % i], int(g["res%d" % i]) - 1)
        for key, val in zip(g["keys%d" % i], g["vals%d" % i]):
            key = str(key)
            if "PSNR" in key:
                assert abs(m[key] - float(val)) < 1e-3, (key, m[key], float(val))          # pc_error prints 4 decimals
            else:
                assert abs(m[key] - float(val)) <= 1e-5 * max(1.0, abs(float(val))), (key, m[key], float(val))


def test_d2_metric_vs_pc_error_golden(golden):
    """Point-to-plane figures (pcgc_d2_*) against pc_error_d run with `-n A`: two seeded voxel clouds with noisy,
    non-unit normals and two hand-made tie cases (equal-distance neighbours, shared normal transfer)."""
    from pcgcv1_amd import metrics
    g = golden("pc_error_d2.npz")
    keys = [str(k) for k in g["keys"]]
    for i in range(int(g["n_cases"])):
        m = metrics.pc_error(g["a%d" % i], g["b%d" % i], g["na%d" % i], int(g["res%d" % i]) - 1)
        for key, val in zip(keys, g["vals%d" % i]):
            val = float(val)
            if "PSNR" in key:
                assert abs(m[key] - val) < 1e-3, (i, key, m[key], val)
            else:
                assert abs(m[key] - val) <= 2e-5 * max(1.0, abs(val)), (i, key, m[key], val)       # 6 significant digits printed


def test_cli_and_eval_end_to_end(tmp_path, monkeypatch):
    """test.py compress / decompress (reference flags) through files, plus one eval.py-style rate point."""
    from pcgcv1_amd import eval as pe
    from pcgcv1_amd import test as cli
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    ply = tmp_path / "tiny_vox7.ply"
    iop.write_ply_data(str(ply), pts)
    monkeypatch.chdir(tmp_path)
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20"])
    for ext in ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos"):
        assert (tmp_path / "compressed" / ("tiny_vox7." + ext)).exists()
    cli.main(["decompress", "compressed/tiny_vox7", "--ckpt_dir=synthetic:7:sparse"])
    rec = iop.load_ply_data(str(tmp_path / "tiny_vox7_rec.ply"))
    nums = np.frombuffer((tmp_path / "compressed" / "tiny_vox7.pointnums").read_bytes(), np.uint16)
    assert len(rec) >= int(nums.sum()) and rec.min() >= 0 and rec.max() < 128       # >=: ties at the threshold are kept
    r = pe.test_hyper(pts, model, "synthetic:7:sparse", min_num=20, resolution=127)
    assert r["n_points_out"] == len(rec) and r["bpp"] > 0 and np.isfinite(r["d1_psnr"])
    assert abs(r["bpp"] - sum(r["bpp_" + k] for k in ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos"))) < 1e-9


def test_cli_runs_the_pipelined_path(tmp_path, monkeypatch, capsys):
    """A cloud of >= 96 cubes through test.py takes the batched two-pipeline branch that bench.py times
    (transform._run_pipes), not the per-stage synchronised one, and writes the same files as the staged branch."""
    from pcgcv1_amd import test as cli
    pts = synthetic.make_cloud(seed=1300, res=512, n_shells=10)
    ply = tmp_path / "big_vox9.ply"
    iop.write_ply_data(str(ply), pts)
    monkeypatch.chdir(tmp_path)
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--cube_size=32", "--min_num=20"])
    out = capsys.readouterr().out
    assert "compress_hyper:" in out and "2 host pipelines" in out, out[-400:]
    files = {e: (tmp_path / "compressed" / ("big_vox9." + e)).read_bytes() for e in ("strings", "strings_head", "strings_hyper")}
    cli.main(["decompress", "compressed/big_vox9", "--ckpt_dir=synthetic:7:sparse", "--cube_size=32"])
    out = capsys.readouterr().out
    assert "decompress_hyper + post process:" in out and "(streamed)" in out and "2 host pipelines" in out, out[-400:]
    rec = (tmp_path / "big_vox9_rec.ply").read_bytes()
    monkeypatch.setenv("PCGC_STAGE_TIMES", "1")                       # the reference's per-stage report: one pipeline
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--cube_size=32", "--min_num=20"])
    out = capsys.readouterr().out
    assert "Analysis Transform:" in out and "1 host pipeline)" in out
    for e, b in files.items():
        assert (tmp_path / "compressed" / ("big_vox9." + e)).read_bytes() == b, e
    cli.main(["decompress", "compressed/big_vox9", "--ckpt_dir=synthetic:7:sparse", "--cube_size=32"])
    assert (tmp_path / "big_vox9_rec.ply").read_bytes() == rec
    # the tail streamed behind the decoder slices (the default above) against postprocess on the whole batch, rho != 1 too
    monkeypatch.delenv("PCGC_STAGE_TIMES")
    for rho in ("1.0", "1.3"):
        recs = []
        for streamed in ("1", "0"):
            monkeypatch.setenv("PCGC_STREAM_TAIL", streamed)
            cli.main(["decompress", "compressed/big_vox9", "--ckpt_dir=synthetic:7:sparse", "--cube_size=32", "--rho=" + rho])
            out = capsys.readouterr().out
            assert ("(streamed)" in out) == (streamed == "1") and "2 host pipelines" in out, out[-400:]
            recs.append((tmp_path / "big_vox9_rec.ply").read_bytes())
        assert recs[0] == recs[1] and (rho != "1.0" or recs[0] == rec)


def test_empty_space_skipping_fuzz():
    """tools/fuzz_skip.py, a short run: random batches of random geometry (planes on tile borders, single voxels, shells, dense
    blocks, empty cubes; ragged batch sizes) with skipping on (virtual tiles / copies) against off: bit-identical latents."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_skip", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             "tools", "fuzz_skip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    prev = os.environ.get("PCGC_SKIP_EMPTY")
    try:
        mod.main(12, 5)
    finally:
        if prev is None:
            os.environ.pop("PCGC_SKIP_EMPTY", None)
        else:
            os.environ["PCGC_SKIP_EMPTY"] = prev


def test_codec_round_trip_fuzz():
    """tools/fuzz_codec.py, a short run: random geometry, batch sizes across the pipeline / slice / chunk boundaries, four
    checkpoints: pipelined strings == staged strings, decoder == encoder-side reconstruction, decode repeatable (bitwise)."""
    import importlib.util
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        spec = importlib.util.spec_from_file_location("fuzz_codec", os.path.join(tools, "fuzz_codec.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.main(8, 11)
    finally:
        sys.path.remove(tools)


def test_streamed_postprocess_matches_postprocess_when_ties_move_the_count(tmp_path):
    """process.StreamedPostprocess writes the slices at offsets that assume sum(k) points; ties at the threshold select
    more, and when that changes the number of digits in the header the file is rewritten: same bytes as postprocess."""
    from pcgcv1_amd import process
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 16, 16, 16, 1), generator=g).cuda()
    x[1].view(-1)[:40] = 9.0                               # 40 voxels tie for the top 3 of cube 1
    nums = np.array([3, 3, 3], np.uint16)                  # 9 points expected, 46 selected
    pos = np.array([[2, 0, 1], [0, 0, 0], [1, 3, 0]], np.int32)
    process.postprocess(str(tmp_path / "a.ply"), x, nums, pos, 1, 16, 1.0, verbose=False)
    for cuts in ([(0, 3)], [(2, 3), (0, 1), (1, 2)]):
        tail = process.StreamedPostprocess(str(tmp_path / "b.ply"), nums, pos, 1, 16, 1.0)
        for lo, hi in cuts:
            tail(lo, hi, x[lo:hi])
        assert tail.finish(verbose=False) == 46
        assert (tmp_path / "b.ply").read_bytes() == (tmp_path / "a.ply").read_bytes()
    tail = process.StreamedPostprocess(str(tmp_path / "c.ply"), nums, pos, 1, 16, 1.0)
    tail(0, 2, x[0:2])
    with pytest.raises(RuntimeError, match="cubes arrived"):
        tail.finish(verbose=False)
    assert not (tmp_path / "c.ply").exists()                 # no half-written file is left behind


def test_rd_harness_eval_csv(tmp_path):
    """eval.py's loop: .ini with two rate sections, input ply with normals -> csv with the reference's columns
    (bpp itemised, D1 / D2 at rho = 1 and the 'optimal' rho)."""
    import csv
    from pcgcv1_amd import eval as pe
    pts = synthetic.make_cloud(seed=6, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    c = pts.mean(0)
    nrm = (pts - c) / np.maximum(np.linalg.norm(pts - c, axis=1, keepdims=True), 1e-9)
    ply = tmp_path / "shell_vox7.ply"
    with open(ply, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(pts))
        for p, n in zip(pts, nrm):
            f.write("%d %d %d %.6f %.6f %.6f\n" % (p[0], p[1], p[2], n[0], n[1], n[2]))
    got_p, got_n = iop.load_ply_normals(str(ply))
    assert np.array_equal(got_p, pts) and np.allclose(got_n, nrm, atol=1e-6)
    ini = tmp_path / "cfg.ini"
    ini.write_text("[DEFAULT]\ncube_size = 64\nmin_num = 20\n\n[R1]\nscale = 1.0\nckpt_dir = synthetic:7:sparse\nrho_d1 = 1.0\nrho_d2 = 1.2\n\n"
                   "[R2]\nscale = 1.0\nckpt_dir = synthetic:8:sparse\nrho_d1 = 0.9\nrho_d2 = 1.0\n")
    rows = pe.eval(str(ply), str(tmp_path / "results"), str(ini), 128)
    assert [r["rate"] for r in rows] == ["R1", "R2"]
    with open(tmp_path / "results" / "shell_vox7.csv") as f:
        table = list(csv.DictReader(f))
    assert len(table) == 2
    for r, t in zip(rows, table):
        for k in ("bpp", "bpp_strings", "bpp_strings_hyper", "bpp_strings_head", "bpp_pointsnums", "bpp_cubepos", "ori_points",
                  "mseF,PSNR (p2point)", "mseF,PSNR (p2plane)", "optimal D1 PSNR", "optimal D2 PSNR", "rho_d1", "rho_d2"):
            assert k in t and np.isfinite(float(t[k])), k
        assert r["ori_points"] == len(pts)
        assert abs(r["bpp"] - (r["bpp_strings"] + r["bpp_strings_hyper"] + r["bpp_strings_head"] + r["bpp_pointsnums"] + r["bpp_cubepos"])) < 3e-4
    assert rows[0]["optimal D1 PSNR"] == rows[0]["mseF,PSNR (p2point)"]            # rho_d1 = 1 reuses the rho = 1 measurement
    assert rows[1]["optimal D2 PSNR"] == rows[1]["mseF,PSNR (p2plane)"]


HYPER_CKPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "checkpoints", "hyper")
SIX_RATES = ["a0.75b3.00", "a2.00b3.00", "a3.50b3.00", "a6.00b3.00", "a10.00b3.00", "a16.00b3.00"]


@pytest.mark.skipif(not all(os.path.isdir(os.path.join(HYPER_CKPT, r)) for r in SIX_RATES), reason="the six trained hyper checkpoints are not all present")
def test_config3_four_frames_six_rate_points(tmp_path):
    """BASELINE configs[2] at its real shape: 4 vox10-sized frames x the reference's SEVEN hyper rate sections (R1 = a0.75b3 at
    scale 5/8, R2 ... R7 = the six checkpoints a0.75b3 ... a16b3, eval_ablation_studies.py:71-77) through the reference's
    driver flow — default .ini written per frame, compress / container / decompress, the rho search for the best D1 / D2
    written back into the .ini (152-205), three reconstructions, csv.  The checkpoints are the six trained with this
    repository (checkpoints/README.md); the frames are seeded synthetic clouds the training never saw (no 8iVFB frame exists
    offline).  Asserted per frame: an RD CURVE — bpp and D1 (rho = 1) strictly increasing over R2 ... R7, R1 below R2 in rate;
    the searched rho values sit on the reference's ladders and the optimal PSNRs are >= the rho = 1 ones; the bpp
    itemisation adds up; the csv has the reference's columns.  Once: decoder == encoder-side reconstruction for every
    checkpoint (the reference substitutes the encoder's tensor, eval.py:96-100), D1 against an independent KD-tree."""
    import configparser
    import csv
    import time
    from scipy.spatial import cKDTree
    from pcgcv1_amd import eval as pe
    from pcgcv1_amd import eval_ablation_studies as abl
    t_start = time.time()
    frame0 = synthetic.make_cloud(seed=2000)
    for r in SIX_RATES:
        ckpt = os.path.join(HYPER_CKPT, r)
        cubes, _, _ = process.preprocess_points(frame0, 1.0, 64, 64)
        out = transform.compress_hyper(cubes, model, ckpt, decompress=True)
        assert torch.equal(transform.decompress_hyper(*out[:8], model, ckpt), out[8]), ckpt
    root = tmp_path / "results"
    curves = []
    for f in range(4):
        pts = synthetic.make_cloud(seed=2000 + f)
        assert 600000 < len(pts) < 1100000                                   # vox10-sized: longdress has 857 966 points
        c = pts.mean(0)
        nrm = (pts - c) / np.maximum(np.linalg.norm(pts - c, axis=1, keepdims=True), 1e-9)
        ply = tmp_path / ("frame%d_vox10.ply" % f)
        with open(ply, "w") as fh:
            fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                     "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(pts))
            np.savetxt(fh, np.concatenate([pts.astype(np.float64), nrm], 1), fmt="%d %d %d %.6f %.6f %.6f")
        rows = abl.eval(str(ply), str(root), 1024, "hyper", 64, "models.model_voxception", None, "", ckpt_root=HYPER_CKPT)
        assert [r["rate"] for r in rows] == ["R1", "R2", "R3", "R4", "R5", "R6", "R7"]
        cfg = configparser.ConfigParser()
        cfg.read(root / "cfg" / ("frame%d_vox10.ini" % f))
        assert cfg.sections() == [r["rate"] for r in rows] and float(cfg.get("R1", "scale")) == 0.625
        assert [os.path.basename(cfg.get(s_, "ckpt_dir").rstrip("/")) for s_ in cfg.sections()] == [SIX_RATES[0]] + SIX_RATES
        with open(root / "csv" / ("frame%d_vox10.csv" % f)) as fh:
            table = list(csv.DictReader(fh))
        assert len(table) == 7
        for r, t in zip(rows, table):
            for k in ("bpp", "bpp_strings", "bpp_strings_hyper", "bpp_strings_head", "bpp_pointsnums", "bpp_cubepos", "ori_points",
                      "mseF,PSNR (p2point)", "mseF,PSNR (p2plane)", "optimal D1 PSNR", "optimal D2 PSNR", "rho_d1", "rho_d2"):
                assert k in t and np.isfinite(float(t[k])), (f, r["rate"], k)
            assert r["ori_points"] == len(pts)
            assert abs(r["bpp"] - (r["bpp_strings"] + r["bpp_strings_hyper"] + r["bpp_strings_head"] + r["bpp_pointsnums"]
                                   + r["bpp_cubepos"])) < 3e-4                    # each term is rounded to 4 decimals
            # the rho search: values from the reference's ladders, written back, never worse than rho = 1 where the walk passed it
            assert r["rho_d1"] in pe.RHOS_D1 and r["rho_d2"] in pe.RHOS_D2
            assert float(cfg.get(r["rate"], "rho_d1")) == r["rho_d1"] and float(cfg.get(r["rate"], "rho_d2")) == r["rho_d2"]
        # every search walked its ladder the way the reference's loop does (eval_ablation_studies.py:156-172): in order, the
        # running maximum starting at 0 after the first entry (so the second entry always replaces the first, sic), stopping
        # at the first PSNR below the maximum, choosing the last rho before it — replayed here on the logged PSNRs
        log, searches = pe.eval.last_search_log, []
        for item, i, rho, psnr in log:
            if i == 0:
                searches.append((item, []))
            searches[-1][1].append((rho, psnr))
        assert len(searches) == 14 and [s_[0] for s_ in searches] == ["mseF,PSNR (p2point)", "mseF,PSNR (p2plane)"] * 7
        for k, (item, walk) in enumerate(searches):
            ladder = pe.RHOS_D1 if k % 2 == 0 else pe.RHOS_D2
            assert [w[0] for w in walk] == ladder[:len(walk)]
            best, mx = None, 0.0
            for i, (rho, psnr) in enumerate(walk):
                mx = 0.0 if i == 0 else max(psnr, mx)
                if psnr < mx:
                    assert i == len(walk) - 1                              # the walk ended exactly where the loop breaks
                    break
                best = rho
            else:
                assert len(walk) == len(ladder)                            # ... or ran off the end of the ladder
            assert best == rows[k // 2]["rho_d1" if k % 2 == 0 else "rho_d2"], (f, k, walk)
        bpp = [r["bpp"] for r in rows]
        d1 = [r["mseF,PSNR (p2point)"] for r in rows]
        curves.append(list(zip(bpp, d1, [r["optimal D1 PSNR"] for r in rows], [r["optimal D2 PSNR"] for r in rows])))
        assert all(b2 > b1 for b1, b2 in zip(bpp[1:-1], bpp[2:])), (f, bpp)     # R2 < R3 < ... < R7 in rate
        assert all(q2 > q1 for q1, q2 in zip(d1[1:-1], d1[2:])), (f, d1)       # ... and in D1
        assert bpp[0] < bpp[1] and d1[0] < d1[1]                               # R1: the lowest checkpoint on the 5/8 down-scaled cloud
        if f == 0:      # D1 of one rate point against an independent nearest-neighbour computation
            ck = os.path.join(HYPER_CKPT, SIX_RATES[3])
            cubes_d, pos, nums, n, _ = pe.rate_point(pts, model, ck, 1.0, 64, 64)
            rec = np.unique(np.rint(process.postprocess_points(cubes_d, nums, pos, 1.0, 64, 1.0)).astype(np.int32), axis=0)
            da = cKDTree(rec).query(pts.astype(np.float64))[0] ** 2
            db = cKDTree(pts).query(rec.astype(np.float64))[0] ** 2
            psnr = 10 * np.log10(3 * 1023.0 ** 2 / max(da.mean(), db.mean()))
            assert abs(rows[4]["mseF,PSNR (p2point)"] - psnr) < 1e-3, (rows[4]["mseF,PSNR (p2point)"], psnr)
    for f, cv in enumerate(curves):
        print("frame %d: " % f + "  ".join("%.4f bpp %.2f / %.2f / %.2f dB" % p for p in cv))
    print("config 3 (4 frames x 7 rate sections, rho search + eval + metrics): %.1f s" % (time.time() - t_start))


def test_config1_single_cube_factorized_path(tmp_path, monkeypatch):
    """BASELINE configs[0]: one 64^3 occupancy cube through the factorized model_voxception path
    (transform.py:24-87): analysis -> 16-channel EntropyBottleneck string -> synthesis, against the oracle's
    analysis / rint / synthesis; then the same through test.py --mode=factorized files."""
    from pcgcv1_amd import test as cli
    w = synthetic.make_weights(seed=21, profile="sparse")
    checkpoint._CACHE["cfg1"] = w
    x = synthetic.make_cubes(seed=21, n_cubes=1, cube_size=64)
    strings, min_v, max_v, shape = transform.compress_factorized(x, model, "cfg1")
    assert tuple(shape) == (1, 16, 16, 16, 16) and isinstance(strings, (bytes, bytearray)) and len(strings) > 0
    y_ref = onets.analysis_transform(onets.sub(w, "analysis_transform"), x)
    q_ref = np.rint(y_ref)
    eb = transform.get_codec(model, "cfg1").entropy_bottleneck_y("cfg1")
    y_dec = eb.decompress(strings, min_v, max_v, shape, 16).cpu().numpy()
    near_tie = np.abs(y_ref - np.floor(y_ref) - 0.5) < 1e-4                # rint may flip where y sits on a .5 boundary
    assert np.array_equal(y_dec[~near_tie], q_ref[~near_tie]) and near_tie.mean() < 1e-3
    assert (min_v, max_v) == (int(y_dec.min()), int(y_dec.max()))
    x_dec = transform.decompress_factorized(strings, min_v, max_v, shape, model, "cfg1").cpu().numpy()
    x_ref = onets.synthesis_transform(onets.sub(w, "synthesis_transform"), y_dec)
    _close(x_dec, x_ref, "factorized decode logits", tol=1e-4)
    # CLI, files in the factorized container (inout_bitstream.py:10-70)
    pts = synthetic.make_cloud(seed=9, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    ply = tmp_path / "f_vox7.ply"
    iop.write_ply_data(str(ply), pts)
    monkeypatch.chdir(tmp_path)
    cli.main(["compress", str(ply), "--mode=factorized", "--ckpt_dir=synthetic:7:sparse", "--min_num=20"])
    for ext in ("strings", "pointnums", "cubepos"):                      # the factorized container has no head file
        assert (tmp_path / "compressed" / ("f_vox7." + ext)).exists()
    cli.main(["decompress", "compressed/f_vox7", "--mode=factorized", "--ckpt_dir=synthetic:7:sparse"])
    rec = iop.load_ply_data(str(tmp_path / "f_vox7_rec.ply"))
    assert len(rec) > 0 and rec.min() >= 0 and rec.max() < 128


def test_eval_factorized_mode(tmp_path):
    """eval.py --mode=factorized (eval.py:45-75, 188-189; eval_ablation_studies.py:54-68): the rate loop over a config .ini
    through compress_factorized + the three-file container + decompress_factorized on seeded 16-channel bottlenecks — csv
    with the reference's columns, bpp itemised without hyper / head terms, the rho search written back, the decoded
    cubes equal to the direct compress_factorized / decompress_factorized round trip; and the default config of both
    factorized model families."""
    import configparser
    import csv
    from pcgcv1_amd import eval as pe
    from pcgcv1_amd import eval_ablation_studies as abl
    from pcgcv1_amd.models import model_simple
    pts = synthetic.make_cloud(seed=9, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    c = pts.mean(0)
    nrm = (pts - c) / np.maximum(np.linalg.norm(pts - c, axis=1, keepdims=True), 1e-9)
    ply = tmp_path / "f_vox7.ply"
    with open(ply, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(pts))
        np.savetxt(fh, np.concatenate([pts.astype(np.float64), nrm], 1), fmt="%d %d %d %.6f %.6f %.6f")
    ini = tmp_path / "f_vox7.ini"
    ini.write_text("[DEFAULT]\ncube_size = 64\nmin_num = 20\nresolution = 128\n"
                   "[R1]\nscale = 1.0\nckpt_dir = synthetic:7:sparse\n[R2]\nscale = 1.0\nckpt_dir = synthetic:8:dense\n")
    rows = pe.eval(str(ply), str(tmp_path / "csv"), str(ini), 128, mode="factorized", cube_size=64)
    assert [r["rate"] for r in rows] == ["R1", "R2"]
    with open(tmp_path / "csv" / "f_vox7.csv") as fh:
        table = list(csv.DictReader(fh))
    assert len(table) == 2
    cfg = configparser.ConfigParser()
    cfg.read(ini)
    for r, t in zip(rows, table):
        for k in ("bpp", "bpp_strings", "bpp_strings_hyper", "bpp_strings_head", "bpp_pointsnums", "bpp_cubepos", "ori_points",
                  "mseF,PSNR (p2point)", "mseF,PSNR (p2plane)", "optimal D1 PSNR", "optimal D2 PSNR", "rho_d1", "rho_d2"):
            assert k in t and np.isfinite(float(t[k])), (r["rate"], k)
        assert r["bpp_strings_hyper"] == 0 and r["bpp_strings_head"] == 0 and r["bpp_strings"] > 0      # eval.py:69-70
        assert abs(r["bpp"] - (r["bpp_strings"] + r["bpp_pointsnums"] + r["bpp_cubepos"])) < 2e-4
        assert r["ori_points"] == len(pts)
        assert r["rho_d1"] in pe.RHOS_D1 and r["rho_d2"] in pe.RHOS_D2
        assert float(cfg.get(r["rate"], "rho_d1")) == r["rho_d1"] and float(cfg.get(r["rate"], "rho_d2")) == r["rho_d2"]
    # one rate point against the direct calls: same bytes in the strings file, same decoded cubes
    cubes, pos, nums = process.preprocess_points(pts, 1.0, 64, 20)
    strings, min_v, max_v, shape = transform.compress_factorized(cubes, model, "synthetic:7:sparse")
    direct = transform.decompress_factorized(strings, min_v, max_v, shape, model, "synthetic:7:sparse")
    cubes_d, pos_d, nums_d, n, bpps = pe.rate_point(pts, model, "synthetic:7:sparse", 1.0, 64, 20, rootdir=str(tmp_path / "c"),
                                                    mode="factorized")
    assert torch.equal(cubes_d, direct) and np.array_equal(nums_d, nums) and n == len(pts)
    assert (tmp_path / "c" / "x.strings").read_bytes()[12:] == bytes(strings)
    assert bpps[1] == round(8 * (12 + len(strings)) / float(len(pts)), 4) and bpps[2] == 0 and bpps[3] == 0
    out = pe.test_factorized(pts, model, "synthetic:7:sparse", min_num=20, resolution=127)
    assert out["bpp"] == bpps[0] and np.isfinite(out["d1_psnr"]) and out["n_cubes"] == len(nums)
    # default configs (eval_ablation_studies.py:54-68): voxception R1 (a2b3 at 0.625) ... R6 (a16b3); simple a1b3 ... a6b3
    _, f1 = pe.set_default_config(str(ply), str(tmp_path / "cfgv"), 128, "factorized", 64)
    c1 = configparser.ConfigParser()
    c1.read(f1)
    assert c1.sections() == ["R1", "R2", "R3", "R4", "R5", "R6"] and float(c1.get("R1", "scale")) == 0.625
    assert [os.path.basename(c1.get(s_, "ckpt_dir").rstrip("/")) for s_ in c1.sections()] == ["a2b3", "a2b3", "a4b3", "a6b3", "a10b3", "a16b3"]
    assert all("checkpoints/factorized" in c1.get(s_, "ckpt_dir") for s_ in c1.sections())
    _, f2 = pe.set_default_config(str(ply), str(tmp_path / "cfgs"), 128, "factorized", 64, modelname="models.model_simple")
    c2 = configparser.ConfigParser()
    c2.read(f2)
    assert [c2.get(s_, "ckpt_dir").rstrip("/").split("/")[-2:] for s_ in c2.sections()] == [["simple", "a%db3" % k] for k in range(1, 7)]
    # the factorized ablation model through the same loop
    ini2 = tmp_path / "s_vox7.ini"
    ini2.write_text("[DEFAULT]\ncube_size = 64\nmin_num = 20\n[R1]\nscale = 1.0\nckpt_dir = synthetic:5:simple\nrho_d1 = 1.0\nrho_d2 = 1.0\n")
    ply2 = tmp_path / "s_vox7.ply"
    ply2.write_bytes(ply.read_bytes())
    rows2 = pe.eval(str(ply2), str(tmp_path / "csv"), str(ini2), 128, mode="factorized", cube_size=64, modelname="models.model_simple")
    assert len(rows2) == 1 and rows2[0]["bpp_strings"] > 0 and np.isfinite(rows2[0]["mseF,PSNR (p2point)"])
    with pytest.raises(ValueError):
        pe.eval(str(ply), str(tmp_path / "csv"), str(ini), 128, mode="nonsense")


def test_cli_edge_cases(tmp_path, monkeypatch):
    """Empty result (every cube under --min_num), a non-default --cube_size, and --scale != 1 through the file CLI."""
    from pcgcv1_amd import test as cli
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(3)
    # 1) 40 scattered points: no cube reaches min_num=64 -> a clear error (the reference fails inside numpy on the
    #    empty cube list, inout_points.py:80-90)
    sparse = np.unique(rng.integers(0, 256, (40, 3)), axis=0).astype(np.int32)
    iop.write_ply_data("empty.ply", sparse)
    with pytest.raises(ValueError, match="min_num"):
        cli.main(["compress", "empty.ply", "--ckpt_dir=synthetic:7:sparse"])
    # zero cubes through the operators themselves: empty in, empty out
    out = transform.compress_hyper(np.zeros((0, 64, 64, 64, 1), np.float32), model, "synthetic:7:sparse")
    assert out[0] == [] and len(out[1]) == 0 and tuple(out[7])[0] == 0
    x0 = transform.decompress_hyper(*out, model, "synthetic:7:sparse")
    assert tuple(x0.shape) == (0, 64, 64, 64, 1)
    # 2) cube_size 32
    pts = synthetic.make_cloud(seed=11, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    iop.write_ply_data("c32.ply", pts)
    cli.main(["compress", "c32.ply", "--ckpt_dir=synthetic:7:sparse", "--cube_size=32", "--min_num=10"])
    cli.main(["decompress", "compressed/c32", "--ckpt_dir=synthetic:7:sparse", "--cube_size=32"])
    nums = np.frombuffer((tmp_path / "compressed" / "c32.pointnums").read_bytes(), np.uint16)
    rec = iop.load_ply_data("c32_rec.ply")
    assert len(nums) > 8 and len(rec) >= int(nums.sum()) and rec.max() < 128
    # 3) scale 0.5: coordinates are halved (rounded, de-duplicated) before partition and doubled back on output
    cli.main(["compress", "c32.ply", "half", "--ckpt_dir=synthetic:7:sparse", "--scale=0.5", "--min_num=10"])
    cli.main(["decompress", "compressed/half", "half_rec.ply", "--ckpt_dir=synthetic:7:sparse", "--scale=0.5"])
    rec = np.loadtxt("half_rec.ply", skiprows=7)
    assert len(rec) > 0 and np.all(rec % 2 == 0) and rec.max() < 130


def test_config5_thousands_of_cubes():
    """BASELINE configs[4]-like: a sparse facade in a 4096^3 grid (scale 0.5 from 8192^3) -> > 2000 cubes of 64^3
    through preprocess -> compress_hyper -> decompress_hyper -> postprocess at full size, checked through
    size-independent properties: the decoder reproduces the encoder-side reconstruction bit for bit, every cube's
    string equals the one obtained by coding that cube in a small batch (batch-slot invariance at scale), the
    container round-trips, and the reconstruction keeps the per-cube point counts."""
    import tempfile
    from pcgcv1_amd.dataprocess import inout_bitstream as bs
    rng = np.random.default_rng(57)
    planes = []
    for axis, off in ((0, 1111), (1, 2503), (2, 3307), (0, 5000)):           # four planar patches in 8192^3
        u = rng.integers(0, 8192, (3_000_000, 2))
        u = u[(u[:, 0] > 1000) & (u[:, 0] < 4200) & (u[:, 1] > 2000) & (u[:, 1] < 5200)]
        p = np.insert(u, axis, off + rng.integers(0, 3, len(u)), axis=1)
        planes.append(p)
    pts8k = np.concatenate(planes).astype(np.int32)
    cubes, cube_positions, points_numbers = process.preprocess_points(pts8k, 0.5, 64, 64)
    B = int(cubes.shape[0])
    assert B > 2000, B
    ck = "synthetic:1300:sparse"
    out = transform.compress_hyper(cubes, model, ck, decompress=True)
    stream, x_enc = out[:8], out[8]
    x_dec = transform.decompress_hyper(*stream, model, ck)
    assert torch.equal(x_dec, x_enc)
    # batch-slot invariance at scale: cubes from the far end of the batch, coded alone
    pick = [0, 1, B // 2, B - 2, B - 1]
    small = transform.compress_hyper(cubes[pick], model, ck)
    for j, i in enumerate(pick):
        assert small[0][j] == stream[0][i] and small[1][j] == stream[1][i] and small[2][j] == stream[2][i], i
    with tempfile.TemporaryDirectory() as d:
        bs.write_binary_files_hyper("house", stream[0], stream[4], points_numbers, cube_positions, stream[1], stream[2], stream[3],
                                    stream[5], stream[6], stream[7], rootdir=d, verbose=False)
        r = bs.read_binary_files_hyper("house", rootdir=d)
    assert list(r[0]) == list(stream[0]) and r[1] == stream[4] and np.array_equal(r[2], points_numbers)
    # the position codec (like tmc3) returns the cubes in its own traversal order; consumers order them by key
    assert np.array_equal(iop.ordered_positions(r[3]), iop.ordered_positions(cube_positions))
    rec = process.postprocess_points(x_dec, r[2], r[3], 0.5, 64, 1.0)
    assert len(rec) >= int(points_numbers.astype(np.int64).sum()) and rec.min() >= 0 and rec.max() < 8192


def test_model_simple_factorized_path(tmp_path, monkeypatch):
    """models/model_simple.py (9^3 / 5^3 stride-2 convs and transposed convs, 32 latent channels) through
    the factorized path: transforms vs the oracle, string round trip, and the CLI with --modelname=models.model_simple."""
    from pcgcv1_amd import test as cli
    from pcgcv1_amd.models import model_simple
    w = synthetic.make_weights_simple(seed=5)
    checkpoint._CACHE["simple5"] = w
    x = synthetic.make_cubes(seed=5, n_cubes=2, cube_size=64)
    a = model_simple.AnalysisTransform().load_weights(w)
    y = a(x).cpu().numpy()
    y_ref = onets.simple_analysis_transform(onets.sub(w, "analysis_transform"), x)
    assert y.shape == (2, 8, 8, 8, 32)
    _close(y, y_ref, "model_simple analysis", tol=2e-5)
    strings, min_v, max_v, shape = transform.compress_factorized(x, model_simple, "simple5")
    assert tuple(shape) == (2, 8, 8, 8, 32) and max_v - min_v >= 2
    eb = transform.get_codec(model_simple, "simple5").entropy_bottleneck_y("simple5", 32)
    assert eb.channels == 32
    y_dec = eb.decompress(strings, min_v, max_v, shape, 32).cpu().numpy()
    near_tie = np.abs(y_ref - np.floor(y_ref) - 0.5) < 1e-4
    assert np.array_equal(y_dec[~near_tie], np.rint(y_ref)[~near_tie])
    x_dec = transform.decompress_factorized(strings, min_v, max_v, shape, model_simple, "simple5").cpu().numpy()
    x_ref = onets.simple_synthesis_transform(onets.sub(w, "synthesis_transform"), y_dec)
    assert x_dec.shape == (2, 64, 64, 64, 1)
    _close(x_dec, x_ref, "model_simple synthesis", tol=1e-4)
    with pytest.raises(ValueError, match="no hyperprior"):
        transform.compress_hyper(x, model_simple, "simple5")
    pts = synthetic.make_cloud(seed=12, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    iop.write_ply_data(str(tmp_path / "s_vox7.ply"), pts)
    monkeypatch.chdir(tmp_path)
    common = ["--mode=factorized", "--modelname=models.model_simple", "--ckpt_dir=synthetic:5:simple"]
    cli.main(["compress", "s_vox7.ply", "--min_num=20"] + common)
    cli.main(["decompress", "compressed/s_vox7"] + common)
    rec = iop.load_ply_data("s_vox7_rec.ply")
    nums = np.frombuffer((tmp_path / "compressed" / "s_vox7.pointnums").read_bytes(), np.uint16)
    assert len(rec) >= int(nums.sum()) > 0 and rec.min() >= 0 and rec.max() < 128


def test_experimental_scheduler_switches_do_not_change_results(tmp_path):
    """PCGC_CHUNKS (cubes per launch at each resolution), PCGC_SLICES (entropy pipeline depth) and PCGC_PIPES (host
    pipelines = threads + streams a batch is split over) are scheduling knobs: same bytes, same logits as the defaults."""
    import os
    import pickle
    import subprocess
    import sys
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, pickle, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from pcgcv1_amd import synthetic, transform\n"
        "from pcgcv1_amd.models import model_voxception as model\n"
        "x = synthetic.make_cubes(seed=2, n_cubes=150)\n"
        "out = transform.compress_hyper(x, model, 'synthetic:1300:sparse')\n"
        "xs = transform.decompress_hyper(*out, model, 'synthetic:1300:sparse').cpu().numpy()\n"
        "pickle.dump((out[0], out[4], np.asarray(out[1]), np.asarray(out[2]), xs[::9]), open(sys.argv[1], 'wb'))\n"
        % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    results = []
    for i, env in enumerate(({}, {"PCGC_CHUNKS": "3,16,32", "PCGC_SLICES": "1", "PCGC_PIPES": "1"}, {"PCGC_CHUNKS": "8,70,70", "PCGC_SLICES": "2", "PCGC_PIPES": "3"},
                             {"PCGC_PIPES": "1"})):
        out = str(tmp_path / ("r%d.pkl" % i))
        e = dict(os.environ)
        e.update(env)
        assert subprocess.run([sys.executable, str(script), out], env=e, timeout=600).returncode == 0, env
        with open(out, "rb") as f:
            results.append(pickle.load(f))
    ref = results[0]
    for i, r in enumerate(results[1:]):
        assert r[0] == ref[0] and r[1] == ref[1] and np.array_equal(r[2], ref[2]) and np.array_equal(r[3], ref[3]), i
        assert np.array_equal(r[4], ref[4]), i


def test_roundtrip_stream_overlaps_clouds_without_changing_them():
    """transform.roundtrip_stream (the encode of cloud k + 1 on its own thread / streams under the decode of cloud k) gives,
    for three different clouds large enough for the two-pipeline path, the bytes and logits of the plain calls."""
    ckpt = "synthetic:1300:sparse"
    clouds = [synthetic.make_cubes(seed=40 + k, n_cubes=n) for k, n in enumerate((120, 97, 130))]
    plain = []
    for x in clouds:
        out = transform.compress_hyper(x, model, ckpt)
        plain.append((out, transform.decompress_hyper(*out, model, ckpt).clone()))
    got = list(transform.roundtrip_stream(iter(clouds), model, ckpt))
    assert len(got) == len(plain)
    for (o, xs), (o_ref, xs_ref) in zip(got, plain):
        assert list(o[0]) == list(o_ref[0]) and o[4] == o_ref[4]
        assert np.array_equal(o[1], o_ref[1]) and np.array_equal(o[2], o_ref[2])
        assert torch.equal(xs, xs_ref)
    assert list(transform.roundtrip_stream(iter(()), model, ckpt)) == []
    # an error in a decode does not leave the encode that runs ahead behind
    bad = transform.roundtrip_stream(iter(clouds[:2]), model, ckpt)
    real = transform.decompress_hyper
    try:
        transform.decompress_hyper = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("decode failed"))
        with pytest.raises(RuntimeError, match="decode failed"):
            next(bad)
    finally:
        transform.decompress_hyper = real
    assert not [t for t in __import__("threading").enumerate() if t.name == "compress-ahead"]


def test_back_to_back_calls_without_synchronisation():
    """Calls that follow each other with device work of the previous one still queued (no synchronisation in between, the
    results only read at the end): the pinned staging buffers a pipeline reuses from call to call (decoded symbols and
    per-cube ranges on their way up) must not be overwritten before the device has read them.  Two different clouds,
    decoded A, B, A, B and encoded in between, against references made one call at a time."""
    ckpt = "synthetic:1300:sparse"
    clouds = [synthetic.make_cubes(seed=70 + k, n_cubes=n) for k, n in enumerate((224, 208))]
    dev_clouds = [torch.from_numpy(x).cuda() for x in clouds]
    ref = []
    for x in dev_clouds:
        out = transform.compress_hyper(x, model, ckpt)
        xs = transform.decompress_hyper(*out, model, ckpt)
        torch.cuda.synchronize()
        ref.append((out, xs.clone()))
    torch.cuda.synchronize()
    got = []
    for rep in range(3):
        for k in (0, 1):
            got.append((k, transform.decompress_hyper(*ref[k][0], model, ckpt)))
        for k in (1, 0):
            got.append((k, transform.compress_hyper(dev_clouds[k], model, ckpt)))
    torch.cuda.synchronize()
    for k, r in got:
        if torch.is_tensor(r):
            assert torch.equal(r, ref[k][1]), "reconstruction of cloud %d differs" % k
        else:
            assert list(r[0]) == list(ref[k][0][0]) and r[4] == ref[k][0][4], "strings of cloud %d differ" % k


def test_loss_module_vs_oracle():
    """pcgcv1_amd.loss (reference names, loss.py:8-93) against oracle/loss.py: BCE means, confusion maps, classification
    metrics (exact counts), focal loss value and gradient."""
    from oracle import loss as oloss
    from pcgcv1_amd import loss
    rng = np.random.default_rng(31)
    pred = (rng.standard_normal((3, 32, 32, 32, 1)) * 4).astype(np.float32)
    label = (rng.random(pred.shape) > 0.96).astype(np.float32)
    e, f = loss.get_bce_loss(pred, label)
    e_ref, f_ref = oloss.get_bce_loss(pred, label)
    assert abs(e - e_ref) <= 1e-5 * abs(e_ref) and abs(f - f_ref) <= 1e-5 * abs(f_ref)
    # classification: logits against labels at th = 0 (loss.py:35-78) and an odd length / another threshold
    for p, l, th in ((pred, label, 0.0), (pred.reshape(-1)[:100003].reshape(-1, 1), label.reshape(-1)[:100003].reshape(-1, 1), 0.5)):
        tp, fp, fn = loss.get_confusion_matrix(p, l, th)
        for got, ref in zip((tp, fp, fn), oloss.get_confusion_matrix(p, l, th)):
            assert got.shape == ref.shape and np.array_equal(got.cpu().numpy(), ref)
        assert loss.classify_counts(p, l, th) == tuple(float(m.sum(dtype=np.float64)) for m in oloss.get_confusion_matrix(p, l, th))
        np.testing.assert_allclose(loss.get_classify_metrics(p, l, th), oloss.get_classify_metrics(p, l, th), rtol=1e-12)
    # nothing predicted, nothing labelled: 0/0 like the reference
    z = np.zeros((1, 8, 8, 8, 1), np.float32)
    assert all(np.isnan(v) for v in loss.get_classify_metrics(z - 1, z))
    # focal loss on probabilities, incl. values outside the clip range and labels that are neither 0 nor 1
    yp = rng.random((2, 16, 16, 16, 1)).astype(np.float32)
    yp.reshape(-1)[:6] = [0.0, 1.0, 5e-4, 0.9995, 0.5, 0.25]
    yt = (rng.random(yp.shape) > 0.9).astype(np.float32)
    yt.reshape(-1)[6] = 0.5
    for gamma, alpha in ((2, 0.9), (1.5, 0.25)):
        v, v_ref = loss.get_focal_loss(yp, yt, gamma, alpha), oloss.get_focal_loss(yp, yt, gamma, alpha)
        assert abs(v - v_ref) <= 2e-5 * abs(v_ref), (v, v_ref)
        g = loss.focal_loss_grad(yp, yt, gamma, alpha).cpu().numpy()
        np.testing.assert_allclose(g, oloss.focal_loss_grad(yp, yt, gamma, alpha), rtol=2e-4, atol=1e-6)
    # the sums do not depend on how the launch is cut: one value for the tensor and for its flattened view
    assert loss.get_focal_loss(yp, yt) == loss.get_focal_loss(yp.reshape(-1), yt.reshape(-1))


def test_one_sided_and_constant_cubes_fit_the_container():
    """A cube whose rounded latents are all > 0 (or all < 0, or all equal) is coded over a support that includes 0, so the
    header byte y_max*16 - y_min of inout_bitstream.py:95-96 can represent it (the reference writes a corrupt byte)."""
    from pcgcv1_amd.dataprocess import inout_bitstream as bs
    rng = np.random.default_rng(4)
    y = np.stack([np.full((4, 4, 4, 16), 3.0), rng.integers(2, 6, (4, 4, 4, 16)), -rng.integers(1, 4, (4, 4, 4, 16)),
                  np.zeros((4, 4, 4, 16))]).astype(np.float32)
    loc = np.zeros_like(y)
    scale = np.full_like(y, 1.5)
    sc = SymmetricConditional()
    strings, mn, mx = sc.compress_cubes(y, loc, scale)
    assert mn.tolist() == [0, 0, -3, 0] and mx.tolist() == [3, 5, 0, 1]
    head = bs.pack_strings_head(strings, mn, mx, np.array([1, 4, 4, 4, 16], np.int32))
    assert len(head) > 0
    dec = sc.decompress_cubes(strings, loc, scale, mn, mx, [1, 4, 4, 4, 16])
    assert np.array_equal(dec.cpu().numpy(), y)


def test_pipelined_codec_is_repeatable():
    """Two host pipelines, their worker pools and streams: twelve steps on a 205-cube batch, every step's strings and
    reconstruction bit-identical to the first (tools/soak.py runs the same check for hundreds of steps)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec_ = importlib.util.spec_from_file_location("soak", os.path.join(root, "tools", "soak.py"))
    soak = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(soak)
    soak.main(12, "sparse")


def _expected_skips(cubes_np, mid=True):
    """Wave tiles the analysis may skip, counted on the host from the occupancy alone (csrc/vrn_row.hip: tile_order_kernel,
    csrc/net.hip: make_empty_responses).  64^3 stage: conv_in tiles are 2 rows x 4 planes at radius 1, the three blocks'
    A / BC tiles 2 rows x 8 planes at radii 2..7.  Behind down_1 (stride 2, one voxel padded behind: output o reads fine
    2o .. 2o + 2 of a radius-7 tensor) the windows are [2o - 7, 2o + 9] fine voxels for down_1 (tiles 2 x 2 on the 32^3 grid)
    and two more fine voxels per side for each of the six launches of the C = 32 blocks (A 4 x 4, BC 2 x 8 for launches of
    more than 16 cubes, 2 x 2 otherwise).  -> (total, per launch)"""
    occ = (cubes_np.reshape(-1, 64, 64, 64) != 0).any(axis=3)          # [B, d, h]: the row holds an occupied voxel
    B = occ.shape[0]
    c = np.zeros((B, 65, 65), np.int64)
    c[:, 1:, 1:] = occ.cumsum(1).cumsum(2)
    cfgs = [(2, 4, 1, 1, 1)] + [(2, 8, r, r, 1) for r in range(2, 8)]
    if mid:
        cfgs.append((2, 2, 7, 9, 2))
        for i in range(6):
            th, ld = (2, 2) if B <= 16 else ((4, 4) if i % 2 == 0 else (2, 8))
            cfgs.append((th, ld, 9 + 2 * i, 11 + 2 * i, 2))
    per_launch = []
    for th, ld, lo, hi, step in cfgs:
        G, n = 64 // step, 0
        for d0 in range(0, G, ld):
            dl, dh = max(step * d0 - lo, 0), min(step * (d0 + ld - 1) + hi, 63)
            for h0 in range(0, G, th):
                hl, hh = max(step * h0 - lo, 0), min(step * (h0 + th - 1) + hi, 63)
                n += int(((c[:, dh + 1, hh + 1] - c[:, dl, hh + 1] - c[:, dh + 1, hl] + c[:, dl, hl]) == 0).sum())
        per_launch.append(n)
    return sum(per_launch), per_launch


def _expected_skips_seg(cubes_np):
    """The same for the segment form (PCGC_SKIP_EMPTY=3; csrc/vrn_seg.hip: seg_order_kernel): conv_in and the six block launches on
    SLOTS of 8 planes x 2 rows x 16 voxels, a slot being skipped when its planes, rows AND voxels dilated by the radius (1 .. 7,
    clipped to the cube) hold no occupied voxel; down_1 and the 32^3 stage as before.  -> (total, per launch)"""
    o = (cubes_np.reshape(-1, 64, 64, 64) != 0)
    B = o.shape[0]
    c3 = np.zeros((B, 65, 65, 65), np.int32)
    c3[:, 1:, 1:, 1:] = o.cumsum(1, dtype=np.int32).cumsum(2, dtype=np.int32).cumsum(3, dtype=np.int32)

    def box(d0, d1, h0, h1, w0, w1):                       # occupied voxels in [d0, d1] x [h0, h1] x [w0, w1], per cube
        d1, h1, w1 = d1 + 1, h1 + 1, w1 + 1
        return (c3[:, d1, h1, w1] - c3[:, d0, h1, w1] - c3[:, d1, h0, w1] - c3[:, d1, h1, w0]
                + c3[:, d0, h0, w1] + c3[:, d0, h1, w0] + c3[:, d1, h0, w0] - c3[:, d0, h0, w0])
    per_launch = []
    for r in range(1, 8):
        n = 0
        for d0 in range(0, 64, 8):
            for h0 in range(0, 64, 2):
                for w0 in range(0, 64, 16):
                    n += int((box(max(d0 - r, 0), min(d0 + 7 + r, 63), max(h0 - r, 0), min(h0 + 1 + r, 63), max(w0 - r, 0), min(w0 + 15 + r, 63)) == 0).sum())
        per_launch.append(n)
    _, rows = _expected_skips(cubes_np)
    per_launch += rows[7:]
    return sum(per_launch), per_launch


def test_empty_space_skipping_is_exact_and_happens(monkeypatch):
    """AnalysisTransform at cube size 64 does not compute wave tiles whose receptive field holds no occupied voxel — conv_in,
    the C = 16 blocks, down_1 and the C = 32 blocks: they equal the net's response to an empty cube there (RowSkip,
    include/pcgc.h).  (a) The latents are BIT-identical with the skipping
    on and off — cubes of the bench cloud, an empty cube, a single voxel in a corner, a dense random cube, a cube with a
    -0.0 voxel; (b) it really skips: the kernels' count of skipped tiles equals the count the host derives from the
    occupancy (every window, every radius, cube faces included), about half of all tiles on the cloud's cubes;
    (c) pcgc_rowocc equals numpy."""
    pts = synthetic.make_cloud(seed=1300)
    cubes, _, _ = process.preprocess_points(pts, 1.0, 64, 64)
    x = cubes[10:26].clone()                                              # two full 8-cube launches of the bench cloud
    special = torch.zeros((8, 64, 64, 64, 1), device=x.device)
    special[1, 0, 0, 0, 0] = 1.0                                          # one voxel in a corner
    special[2, 63, 63, 63, 0] = 1.0
    special[3] = (torch.rand((64, 64, 64, 1), device=x.device) < 0.3).float()
    special[4, 31, 32, :, 0] = 1.0                                        # one full row in the middle
    special[5, 20, 20, 20, 0] = -0.0                                      # -0.0 is not "empty" (its products are -0.0)
    special[6, :, 7, 5, 0] = 1.0                                          # a line along d
    special[7, 40:44, 40:44, 40:44, 0] = 1.0
    x = torch.cat([x, special], 0).contiguous()
    c = transform.get_codec(model, "synthetic:77:dense")
    net = c.analysis_transform
    monkeypatch.setenv("PCGC_SKIP_EMPTY", "0")
    y_all = net(x).clone()
    counter = torch.zeros(1, dtype=torch.int32, device=x.device)
    net.set_skip_counter(counter)
    skipped_by_mode = {}
    try:
        # 1 (default): empty tiles are not written at all, readers take the empty-cube response for them ("virtual" tiles;
        # only the stage's last launch materialises them); 2: every launch copies its empty tiles
        # 3: as 1, with the three C = 16 blocks on slots of 8 planes x 2 rows x 16 voxels (csrc/vrn_seg.hip)
        for mode in ("1", "2", "3"):
            monkeypatch.setenv("PCGC_SKIP_EMPTY", mode)
            counter.zero_()
            y_skip = net(x).clone()
            torch.cuda.synchronize()
            skipped_by_mode[mode] = int(counter.item())
            assert torch.equal(y_all, y_skip), (mode, int((y_all != y_skip).sum()))
            for rep in range(3):
                # tiles that are not written keep whatever the workspace held: poison it (every float a NaN) — a single
                # read of an unwritten tile anywhere in the stage would surface in the latents
                for ws in net._ws.values():
                    ws.fill_(255)
                assert torch.equal(net(x), y_all), (mode, rep)
        # mode 3 with the empty-cube responses copied next to the chunk's tensors (what happens when the net's own copy is out of
        # the buffer window's reach): same latents, same count
        monkeypatch.setenv("PCGC_SKIP_EMPTY", "3")
        monkeypatch.setenv("PCGC_SEG_COPY_EMPTY", "1")
        counter.zero_()
        for ws in net._ws.values():
            ws.fill_(255)
        assert torch.equal(net(x), y_all)
        torch.cuda.synchronize()
        assert int(counter.item()) == skipped_by_mode["3"]
        monkeypatch.delenv("PCGC_SEG_COPY_EMPTY")
        skipped = skipped_by_mode["1"]
        assert skipped_by_mode["2"] == skipped
        counter.zero_()
        monkeypatch.setenv("PCGC_SKIP_EMPTY", "0")
        net(x)
        torch.cuda.synchronize()
        assert int(counter.item()) == 0                                   # switched off: nothing is skipped
    finally:
        net.set_skip_counter(None)
    assert torch.equal(y_all, y_skip)
    xn = x.cpu().numpy()
    xn_occ = xn.copy()
    xn_occ[16 + 5, 20, 20, 20, 0] = 1.0                                   # the -0.0 voxel counts as occupied
    want, per_radius = _expected_skips(xn_occ)
    assert skipped == want, (skipped, want, per_radius)
    want_seg, per_seg = _expected_skips_seg(xn_occ)
    assert skipped_by_mode["3"] == want_seg, (skipped_by_mode["3"], want_seg, per_seg)
    slots = x.shape[0] * 1024
    print("\nsegment form: of %d slots per launch (conv_in, A / BC x 3) %s are computed (row tiles of the blocks: %s)" % (
        slots, ", ".join("%.3f" % (1 - v / slots) for v in per_seg[0:7]), ", ".join("%.3f" % (1 - v / (slots / 4)) for v in per_radius[1:7])))
    tiles = x.shape[0] * (32 * 16 + 6 * 32 * 8 + 16 * 16 + 6 * 64)
    frac_cloud = _expected_skips(xn[:16], mid=False)[0] / float(16 * (32 * 16 + 6 * 32 * 8))
    assert 0.3 < frac_cloud < 0.8, frac_cloud
    print("\nempty-space skipping: %d of %d wave tiles skipped (64^3 stage: %.1f %% on the bench cloud's cubes), latents bit-identical; per launch %r"
          % (skipped, tiles, 100 * frac_cloud, per_radius))
    # (c) the row-occupancy words
    ro = torch.zeros(x.shape[0] * 64, dtype=torch.int64, device=x.device)
    _lib.check(_lib.hip().pcgc_rowocc(_lib.dptr(x), _lib.dptr(ro), int(x.shape[0]), _lib.stream()), "pcgc_rowocc")
    occ = (xn_occ.reshape(-1, 64, 64, 64) != 0).any(axis=3).reshape(-1, 64)
    words = (occ.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert np.array_equal(ro.cpu().numpy().view(np.uint64), words)
    # the whole codec on the trained checkpoint gives the same bytes either way
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "checkpoints", "hyper", "a6.00b3.00")
    if os.path.isdir(d):
        monkeypatch.setenv("PCGC_SKIP_EMPTY", "0")
        o0 = transform.compress_hyper(cubes, model, d)
        for mode in ("1", "2", "3"):
            monkeypatch.setenv("PCGC_SKIP_EMPTY", mode)
            o1 = transform.compress_hyper(cubes, model, d)
            assert list(o0[0]) == list(o1[0]) and bytes(o0[4]) == bytes(o1[4]), mode


# Frozen from commit 042b3e5 (the parent of the workspace-plan refactor of csrc/net.hip) on an MI355X.
_PLAN_MODES = (("0", None), ("1", None), ("2", None), ("3", None), ("3", "1"))        # PCGC_SKIP_EMPTY, PCGC_SEG_COPY_EMPTY
_PLAN_LATENTS_SHA = "00eb7807e16dad55511f24413f9de3f9395da3c4c06eb58f8d362399523740e2"
_PLAN_SYNTHESIS_SHA = "cda786f4fbe98dc0a884d6e09b3dc0b5c1158ac40131bf6e7bfb78a8e541a28b"
_PLAN_ROW_TILES = "409c8fe491f92a4ef0f0fe2da2058aa68b907343683e3c1e0c6f3ab9525179b6"
_PLAN_SLOTS = "ad66e7622e70a66d790317bd2340e09474269234877149c49ab49b1d29933d68"
_PLAN_LAUNCHES_SHA = {          # (PCGC_SKIP_EMPTY, PCGC_SEG_COPY_EMPTY) -> sha256 of the (layer, kernel, B, Din) rows, analysis then synthesis
    ("0", None): _PLAN_ROW_TILES, ("1", None): _PLAN_ROW_TILES, ("2", None): _PLAN_ROW_TILES, ("3", None): _PLAN_SLOTS, ("3", "1"): _PLAN_SLOTS,
}
_PLAN_WORKSPACE_BYTES = {       # (net, B, D, PCGC_SKIP_EMPTY) -> pcgc_net_workspace_bytes, default chunk sizes; the parent's value beside it
    ("analysis", 1, 64, "0"): 126968576,            # 126969684
    ("analysis", 7, 64, "0"): 335129344,            # 335130444
    ("analysis", 41, 64, "0"): 611883008,           # 611884148
    ("analysis", 205, 64, "0"): 1655370240,         # 1655371332
    ("analysis", 1, 64, "3"): 126968576,            # 126969684
    ("analysis", 7, 64, "3"): 335129344,            # 335130444
    ("analysis", 41, 64, "3"): 1485346816,          # 1485347956
    ("analysis", 205, 64, "3"): 2360013312,         # 2360014404
    ("synthesis", 7, 16, "3"): 235071624,           # 235071880
    ("synthesis", 205, 16, "3"): 1335168984,        # 1335169240
    ("hyper_encoder", 205, 16, "3"): 60457216,      # 60457216
    ("hyper_decoder", 205, 8, "3"): 167936256,      # 167936256
}


def test_net_plan_is_the_parents(monkeypatch):
    """The host-side plan of pcgc_net_forward (csrc/net_plan.h: workspace regions, chunk views, launch numbers) computes what
    the hand-written layout before it computed.  Seven 64^3 cubes (five of the bench cloud, an empty one, a single voxel in
    a corner) with PCGC_CHUNKS=2,3,5 give two super chunks (5 + 2), ragged last chunks at all three resolutions and
    equal-size 64^3 chunks 2 / 2 / 1 and 2.  For every skip mode, on a poisoned workspace: (a) the analysis latents, (b) the
    synthesis output for them, (c) the launch sequences of both transforms are the parent commit's, frozen as sha256; (d) the
    workspace sizes are pinned, none above the parent's."""
    import hashlib

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def launches(net, x):
        net.set_profiling(True)
        try:
            y = net(x).clone()
            torch.cuda.synchronize()
            rows = ["%d %s %d %d" % (r["layer"], r["kernel"], r["B"], r["Din"]) for r in net.profile_report()]
        finally:
            net.set_profiling(False)
        return y, rows

    pts = synthetic.make_cloud(seed=1300)
    cubes, _, _ = process.preprocess_points(pts, 1.0, 64, 64)
    special = torch.zeros((2, 64, 64, 64, 1), device=cubes.device)
    special[1, 0, 0, 0, 0] = 1.0
    x = torch.cat([cubes[10:15], special], 0).contiguous()
    c = transform.get_codec(model, "synthetic:77:dense")
    ana, syn = c.analysis_transform, c.synthesis_transform
    monkeypatch.setenv("PCGC_CHUNKS", "2,3,5")
    got = {}
    for mode, copy in _PLAN_MODES:
        monkeypatch.setenv("PCGC_SKIP_EMPTY", mode)
        if copy is None:
            monkeypatch.delenv("PCGC_SEG_COPY_EMPTY", raising=False)
        else:
            monkeypatch.setenv("PCGC_SEG_COPY_EMPTY", copy)
        ana(x), syn(ana(x))                                               # the workspaces exist: poison them
        for net in (ana, syn):
            for ws in net._ws.values():
                ws.fill_(255)
        y, rows_a = launches(ana, x)
        xs, rows_s = launches(syn, y)
        got[(mode, copy)] = (sha(y), sha(xs), hashlib.sha256("\n".join(rows_a + ["--"] + rows_s).encode()).hexdigest(), rows_a, rows_s)
        print("plan mode %s copy %s: latents %s synthesis %s launches %s (%d + %d rows)" % (mode, copy, got[(mode, copy)][0], got[(mode, copy)][1],
                                                                                           got[(mode, copy)][2], len(rows_a), len(rows_s)))
    monkeypatch.delenv("PCGC_SEG_COPY_EMPTY", raising=False)
    monkeypatch.delenv("PCGC_CHUNKS")
    lib = _lib.hip()
    sizes = {}
    for name, net, shapes, modes in (("analysis", ana, [(1, 64), (7, 64), (41, 64), (205, 64)], ("0", "3")), ("synthesis", syn, [(7, 16), (205, 16)], ("3",)),
                                     ("hyper_encoder", c.hyper_encoder, [(205, 16)], ("3",)), ("hyper_decoder", c.hyper_decoder, [(205, 8)], ("3",))):
        for mode in modes:
            monkeypatch.setenv("PCGC_SKIP_EMPTY", mode)
            for B, D in shapes:
                sizes[(name, B, D, mode)] = int(lib.pcgc_net_workspace_bytes(net._handle, B, D))
                print("plan workspace %r: %d," % ((name, B, D, mode), sizes[(name, B, D, mode)]))
    for key in _PLAN_MODES:
        y_sha, xs_sha, l_sha, rows_a, rows_s = got[key]
        assert y_sha == _PLAN_LATENTS_SHA, key
        assert xs_sha == _PLAN_SYNTHESIS_SHA, key
        assert l_sha == _PLAN_LAUNCHES_SHA[key], (key, rows_a, rows_s)
    assert sizes == _PLAN_WORKSPACE_BYTES
