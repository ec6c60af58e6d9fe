"""-m gpu: the codec at cube sizes other than 64 (--cube_size) against the CPU oracle.

At any size but 64 the four networks leave the row kernels (csrc/net.hip: forward_autoencoder, forward_chunk, Exec::vrn):
the C = 16 blocks run on the two VALU kernels of vrn_valu.hip, the C = 32 blocks on the fused tap-split MFMA kernels of
vrn_mfma.hip (fuse 1 / fuse 2), conv_in / deconv_out on conv_valu.hip, the resamplers on conv_mfma.hip or conv_direct.hip and
the hyper networks on the generic layer path.  The sharding and CLI tests run those sizes but compare the HIP path with
itself; here every transform is compared with oracle/nets.py, on the default plan and on the direct kernels (set_algo(1): a
wrong fast kernel shows on the first only, a wrong plan on both), the profile report must name the kernels the plan is meant
to pick, the results must not depend on the run, the batch slot or the chunking, and the entropy stage must produce the
oracle's bytes from segments of 8^3 * 16 and 4^3 * 16 rows.  Inputs and references: tests/_cube_sizes.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _cube_sizes as cz                                                  # noqa: E402
from oracle import entropy as oent                                        # noqa: E402
from oracle import nets as onets                                          # noqa: E402
from oracle import points as opoints                                      # noqa: E402
from pcgcv1_amd import checkpoint, transform                              # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                    # noqa: E402
from pcgcv1_amd.models import model_voxception as model                   # noqa: E402

# cube size, cubes: 96 = 6 tiles of the VALU kernels along w and 3 of the fused kernels at 48^3; 128 = the fused kernels at
# 64^3 and the C = 64 blocks on the generic MFMA path at 32^3 (first sheet only)
SIZES = [(16, cz.N_CUBES), (32, cz.N_CUBES), (96, cz.N_CUBES), (128, 1)]
TOL_AE, TOL_HYPER = 2e-5, 1e-5        # test_gpu_parity.py's: depth and terms per output do not depend on the cube size
NETS = ("analysis_transform", "synthesis_transform", "hyper_encoder", "hyper_decoder")


def _close(a, b, what, tol):
    """test_gpu_parity._close; the figure is printed before it is judged."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    print("%s: max|diff| %.3g (bound %.3g)" % (what, err, tol * scale))
    assert err <= tol * scale, "%s: max|diff| %.3g > %.3g" % (what, err, tol * scale)


def _dev(a):
    return torch.tensor(a, dtype=torch.float32).cuda()                   # a copy: the shared arrays are read-only


@pytest.fixture(scope="module")
def codec():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    checkpoint._CACHE[cz.CKPT] = cz.weights()
    return transform.get_codec(model, cz.CKPT)


def _nets(c):
    return [getattr(c, n) for n in NETS]


# ---------------------------------------------------------------------------------------------------------------------
# 1. every transform against the oracle, default plan and direct kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("cs,n", SIZES)
def test_transforms_vs_oracle(codec, cs, n, algo):
    x = cz.batch(cs)[:n]
    y_ref, z_ref, x_ref = cz.oracle_y(cs, n), cz.oracle_z(cs, n), cz.oracle_x(cs, n)
    loc_ref, scale_ref = cz.oracle_loc_scale(cs, n)
    tag = "cube size %d, %s" % (cs, "direct path" if algo else "default path")
    try:
        for net in _nets(codec):
            net.set_algo(algo)
        y = codec.analysis_transform(_dev(x)).cpu().numpy()
        z = codec.hyper_encoder(_dev(y_ref)).cpu().numpy()
        loc, scale = (t.cpu().numpy() for t in codec.hyper_decoder(_dev(np.rint(z_ref)), lower_bound=1e-9))
        xs = codec.synthesis_transform(_dev(np.rint(y_ref))).cpu().numpy()
    finally:
        for net in _nets(codec):
            net.set_algo(0)
    assert y.shape == y_ref.shape and z.shape == z_ref.shape and loc.shape == loc_ref.shape and xs.shape == x_ref.shape
    failures = []
    for got, ref, what, tol in ((y, y_ref, "analysis", TOL_AE), (z, z_ref, "hyper encoder", TOL_HYPER),
                                (loc, loc_ref, "hyper decoder loc", TOL_HYPER), (scale, scale_ref, "hyper decoder scale", TOL_HYPER),
                                (xs, x_ref, "synthesis", TOL_AE)):
        try:
            _close(got, ref, "%s: %s" % (tag, what), tol)
        except AssertionError as e:                                      # every figure is printed before the test fails
            failures.append(str(e))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# 2. the kernels the plan is meant to pick really ran
# ---------------------------------------------------------------------------------------------------------------------
# per cube size: (kernel, Din) of the block kernels both auto-encoder transforms must list, three blocks each.  Read off
# net.hip: C = 16 at D % 16 == 0 -> vrn_valu.hip; C = 32 at (D / 2) % 16 == 0 -> the fused kernels of vrn_mfma.hip
BLOCK_KERNELS = {
    16: [("vrnA", 16), ("vrnBC", 16)],
    32: [("vrnA", 32), ("vrnBC", 32), ("ks1", 16), ("ks2", 16)],
    96: [("vrnA", 96), ("vrnBC", 96), ("ks1", 48), ("ks2", 48)],
    128: [("vrnA", 128), ("vrnBC", 128), ("ks1", 64), ("ks2", 64)],
}


def _profiled(codec, cs, algo):
    """One forward of each transform on the first cube with profiling on -> {net name: rows of the report}."""
    x = _dev(cz.batch(cs)[:1])
    nets = _nets(codec)
    try:
        for net in nets:
            net.set_algo(algo).set_profiling(True)
            net.profile_report()                                         # drop whatever an earlier caller left
        y = codec.analysis_transform(x)
        z = codec.hyper_encoder(y)
        codec.hyper_decoder(torch.round(z), lower_bound=1e-9)
        codec.synthesis_transform(torch.round(y))
        torch.cuda.synchronize()
        return {name: net.profile_report() for name, net in zip(NETS, nets)}
    finally:
        for net in nets:
            net.set_algo(0).set_profiling(False)


@pytest.mark.parametrize("cs", [16, 32, 96, 128])
def test_the_intended_kernels_ran(codec, cs):
    rep = _profiled(codec, cs, 0)
    for name in NETS:
        print("cube size %d, %s: %s" % (cs, name, " ".join("%s:%s@%d" % (r["name"], r["kernel"], r["Din"]) for r in rep[name])))
    for name in NETS:
        assert rep[name], name
        for r in rep[name]:
            assert not r["kernel"].startswith(("row", "seg")), (cs, name, r)
    for name in ("analysis_transform", "synthesis_transform"):
        got = [(r["kernel"], r["Din"]) for r in rep[name]]
        for want in BLOCK_KERNELS[cs]:
            assert got.count(want) == 3, (cs, name, want, got)          # the stage's three blocks, one chunk
    for name, layer in (("analysis_transform", "conv_in"), ("synthesis_transform", "deconv_out")):
        rows = [r for r in rep[name] if r["name"] == layer]
        assert len(rows) == 1 and rows[0]["kernel"] == "valu" and rows[0]["Din"] == cs, (cs, layer, rows)
    if cs == 128:     # the C = 64 blocks at 32^3: no fused form, the generic layers on the MFMA kernels
        for name in ("analysis_transform", "synthesis_transform"):
            assert any(r["kernel"] == "mfma" and r["Din"] == 32 and r["cin"] == 64 for r in rep[name]), (name, rep[name])


@pytest.mark.parametrize("cs", [16, 32, 96, 128])
def test_the_direct_path_is_direct(codec, cs):
    rep = _profiled(codec, cs, 1)
    for name in NETS:
        assert rep[name], name
        assert {r["kernel"] for r in rep[name]} == {"direct"}, (cs, name, sorted({r["kernel"] for r in rep[name]}))


# ---------------------------------------------------------------------------------------------------------------------
# 3. run to run, batch slot, chunking
# ---------------------------------------------------------------------------------------------------------------------
def _pipeline(c, x):
    y = c.analysis_transform(x)
    z = c.hyper_encoder(y)
    loc, scale = c.hyper_decoder(torch.round(z), lower_bound=1e-9)
    return {"analysis": y, "hyper encoder": z, "loc": loc, "scale": scale, "synthesis": c.synthesis_transform(torch.round(y))}


@pytest.mark.parametrize("cs", [32, 96])
def test_results_do_not_depend_on_run_or_batch_slot(codec, cs):
    """The decoder regenerates loc / scale and the reconstruction from another batch size than the encoder used: slot 2 of
    the batch (the third sheet) run alone gives the bits it has in the batch, and a second run gives the bits of the first."""
    x = _dev(cz.batch(cs))
    first = _pipeline(codec, x)
    for name, t in _pipeline(codec, x).items():
        assert torch.equal(t, first[name]), "%s: the second run differs from the first" % name
    y, z = first["analysis"], first["hyper encoder"]
    alone = {"analysis": codec.analysis_transform(x[2:3].contiguous()), "hyper encoder": codec.hyper_encoder(y[2:3].contiguous()),
             "synthesis": codec.synthesis_transform(torch.round(y[2:3]).contiguous())}
    alone["loc"], alone["scale"] = codec.hyper_decoder(torch.round(z[2:3]).contiguous(), lower_bound=1e-9)
    for name, t in alone.items():
        assert torch.equal(t, first[name][2:3]), "%s: slot 2 alone differs from slot 2 of the batch" % name


def test_eleven_cubes_cross_the_chunk_of_the_full_resolution_stage(codec, monkeypatch):
    """Eleven 32^3 cubes (the seven, then the first four again).  The synthesis' full-resolution stage runs 8 cubes per
    launch, so equal_chunk splits them 6 + 5; the analysis' default is 40 per launch (chunk_plan, whatever the cube size),
    so it is also run with PCGC_CHUNKS_A=8,64,256 (read per call), which splits it the same way.  Every repeated cube
    equals its first occurrence, every cube what it is in the batch of seven, and the chunked analysis the unchunked one."""
    cs = 32
    x7 = _dev(cz.batch(cs))
    x11 = torch.cat([x7, x7[:4]]).contiguous()
    seven, eleven = _pipeline(codec, x7), _pipeline(codec, x11)
    monkeypatch.setenv("PCGC_CHUNKS_A", "8,64,256")
    chunked = codec.analysis_transform(x11)
    monkeypatch.delenv("PCGC_CHUNKS_A")
    assert float(eleven["analysis"].abs().max()) > 0 and float(eleven["synthesis"].abs().max()) > 0
    for name, t in eleven.items():
        assert torch.equal(t[7:11], t[0:4]), "%s: a repeated cube differs from its first occurrence" % name
        assert torch.equal(t[:7], seven[name]), "%s: the first seven of eleven differ from the batch of seven" % name
    assert torch.equal(chunked, eleven["analysis"]), "analysis: 6 + 5 cubes per launch differ from one launch of 11"


# ---------------------------------------------------------------------------------------------------------------------
# 4. entropy stage, strings and point selection
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [32, 16])
def test_streams_cross_decode_with_the_oracle(codec, cs):
    """test_gpu_parity.test_streams_cross_decode_with_the_oracle at 32 and 16: pcgc_laplace_cdf on segments of 8^3 * 16 and
    4^3 * 16 rows, the factorized coder on 4^3 * 8 and 2^3 * 8 symbols per cube.  The oracle codes the y, loc, scale and z the
    HIP transforms produced; every string is byte-identical and each side decodes the other's.  Then the decoded logits'
    top-k masks against the oracle's, k = each cube's point count (0 for the empty cube: the reference's values[-0] is the
    smallest candidate, so every voxel is selected, on both sides)."""
    x = np.array(cz.batch(cs)[list(cz.RANGE_SAFE)])
    B, n = len(x), cs // 4
    c, dense = codec, cz.weights()
    ys = c.analysis_transform(_dev(x))
    zs = c.hyper_encoder(ys)
    # ---- z: factorized prior, one string for the batch
    est = onets.sub(dense, "estimator")
    z_np = zs.cpu().numpy()
    s_hip, mn, mx = c.entropy_bottleneck.compress(zs)
    s_ref, mn_r, mx_r = oent.eb_compress(est, z_np)
    assert (mn, mx) == (mn_r, mx_r) and bytes(s_hip) == bytes(s_ref)
    assert np.array_equal(oent.eb_decompress(est, s_hip, mn, mx, z_np.shape), np.rint(z_np))          # oracle decodes HIP
    z_hat = c.entropy_bottleneck.decompress(s_ref, mn_r, mx_r, z_np.shape)                            # HIP decodes oracle
    assert torch.equal(z_hat, torch.round(zs))
    # ---- y: Laplace prior conditioned on the hyper-decoder output, one string per cube
    loc, scale = c.hyper_decoder(z_hat, lower_bound=1e-9)
    sc = c.conditional_entropy_model
    strings, mns, mxs = sc.compress_cubes(ys, loc, scale)
    y_np, loc_np, scale_np = ys.cpu().numpy(), loc.cpu().numpy(), scale.cpu().numpy()
    assert y_np.shape == (B, n, n, n, 16)
    oracle_strings = []
    for b in range(B):
        s_o, mn_o, mx_o = oent.sc_compress(y_np[b:b + 1], loc_np[b:b + 1], scale_np[b:b + 1])
        assert (mn_o, mx_o) == (int(mns[b]), int(mxs[b])), (b, mn_o, mx_o, int(mns[b]), int(mxs[b]))
        assert bytes(s_o) == bytes(strings[b]), "cube %d: HIP and oracle strings differ" % b
        oracle_strings.append(s_o)
        dec = oent.sc_decompress(strings[b], loc_np[b:b + 1], scale_np[b:b + 1], mn_o, mx_o, y_np[b:b + 1].shape)
        assert np.array_equal(dec, np.rint(y_np[b:b + 1]))                                            # oracle decodes HIP
    y_dec = sc.decompress_cubes(oracle_strings, loc, scale, mns, mxs, [1, n, n, n, 16])                # HIP decodes oracle
    assert torch.equal(y_dec, torch.round(ys))
    # ---- point selection on the decoded logits
    logits = c.synthesis_transform(y_dec)
    k = x.sum(axis=(1, 2, 3, 4)).astype(np.int64)
    assert k[cz.RANGE_SAFE.index(cz.EMPTY)] == 0 and k[cz.RANGE_SAFE.index(cz.CORNERS)] == 3
    ref = opoints.select_voxels(logits.cpu().numpy(), k, 1.0)
    assert np.array_equal(iop.select_voxels(logits, k, 1.0).cpu().numpy(), ref.astype(np.uint8))
