"""-m gpu: the 8^3 row kernels of the hyperprior nets (csrc/hyper_row.hip) at every planes-per-wave they launch with.

planes_per_wave(waves_per_cube_at_8, B) starts at 8 output planes per wave and halves while B * waves_per_cube * (8 / ps) < 1024
(every SIMD of the chip gets a wave first).  The kernels with four waves per cube (down8_row_kernel, up8_row_kernel,
conv8_row_kernel<8,16>) therefore run 2 / 4 / 8 planes per wave from B = 64 / 128 / 256, conv8_row_kernel<16,8> (two waves per
cube) from B = 128 / 256 / 512, and with 513 cubes its last workgroup is half empty (1026 waves, four to a workgroup).

Which entry point reaches what:
  * pcgc_net_forward runs the hyper nets in chunks of kHyperChunk = 256 cubes (net_plan.h, net.hip), so a kernel never sees more
    than 256 there: the four-wave kernels reach 2 / 4 / 8 planes per wave at B = 64 / 128 / 256, conv8_row_kernel<16,8> only
    1 / 2 / 4.  B = 512 and 513 run as 256 + 256 (+ 1): what they add is the second and third chunk (their offsets into the
    tensors, a chunk of one cube behind full ones), not a new launch form.
  * pcgc_conv3d_bwd_data of an 8 -> 16 3x3x3 layer at 8^3 (train.hip bwd_data_impl -> launch_hyper_row_conv ->
    launch_conv8_row: the adjoint convolution 16 -> 8) passes B whole: conv8_row_kernel<16,8> at 2 / 4 / 8 planes per wave
    for B = 128 / 256 / 512, and the half-empty last workgroup at B = 513.

Distinct random cubes; the cubes in slots 0, B / 2 and B - 1 must come out as they do alone at B = 1 (the header's
"bit-identical for any batch size / batch slot"), and the B = 1 results are held to the oracle: the nets at the bound
test_transforms_vs_oracle_and_direct holds them to, the layer at the bound test_conv_layer_vs_oracle holds one layer to.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import nets as onets                                          # noqa: E402
from pcgcv1_amd import _lib, synthetic                                    # noqa: E402
from pcgcv1_amd.models import model_voxception as model                   # noqa: E402

ENCODER_B = (64, 128, 256, 512, 513)
DECODER_B = (64, 128, 256)
LOWER_BOUND = 1e-9
ATOL = 1e-5                       # test_gpu_parity.py ATOL: x max(1, max|ref|)


def planes_per_wave(waves_per_cube_at_8, B):
    """hyper_row.hip, restated."""
    ps = 8
    while ps > 1 and B * waves_per_cube_at_8 * (8 // ps) < 1024:
        ps //= 2
    return ps


BWD_B = (128, 256, 512, 513)      # pcgc_conv3d_bwd_data, 8 -> 16 at 8^3: conv8_row_kernel<16,8> with B whole


def _hyper_chunk():
    """kHyperChunk as csrc/net_plan.h has it: the cubes pcgc_net_forward hands one launch of a hyper net."""
    text = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "net_plan.h")).read()
    return int(re.search(r"constexpr int kHyperChunk = (\d+);", text).group(1))


def test_which_planes_per_wave_each_entry_point_reaches():
    """The batch sizes, against the chunking of pcgc_net_forward as the source has it: through the nets every form of the
    four-wave kernels and conv8_row_kernel<16,8> up to 4 planes per wave; 8 planes per wave and the half-empty last workgroup of
    <16,8> only through pcgc_conv3d_bwd_data.  If kHyperChunk changes, this says which sizes to move."""
    chunk = _hyper_chunk()
    through_nets = lambda waves, sizes: {planes_per_wave(waves, min(chunk, B - b0)) for B in sizes for b0 in range(0, B, chunk)}     # noqa: E731
    assert through_nets(4, ENCODER_B) >= {2, 4, 8} and through_nets(4, DECODER_B) >= {2, 4, 8}
    assert through_nets(2, ENCODER_B) == {1, 2, 4}
    assert [planes_per_wave(2, B) for B in (127,) + BWD_B] == [1, 2, 4, 8, 8]
    waves = lambda B: B * 2 * (8 // planes_per_wave(2, B))                                                                          # noqa: E731
    assert waves(513) % 4 == 2 and all(waves(B) % 4 == 0 for B in BWD_B[:-1])


@pytest.fixture(scope="module")
def hyper():
    """The two nets on one synthetic dense checkpoint; per net three probe cubes, their results alone at B = 1, and the fillers
    (distinct random cubes) of the large batches."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    w = synthetic.make_weights(seed=53, profile="dense")
    g = torch.Generator().manual_seed(53)
    enc, dec = model.HyperEncoder().load_weights(w), model.HyperDecoder().load_weights(w)
    y = (torch.randn((max(ENCODER_B) + 3, 16, 16, 16, 16), generator=g) * 2.0).cuda()               # latents: real-valued
    z = torch.round(torch.randn((max(DECODER_B) + 3, 8, 8, 8, 8), generator=g) * 2.0).cuda()         # decoded hyper-latents: integers
    alone_enc = [enc(y[i:i + 1].contiguous()) for i in range(3)]
    alone_dec = [dec(z[i:i + 1].contiguous(), lower_bound=LOWER_BOUND) for i in range(3)]
    return dict(w=w, enc=enc, dec=dec, y=y, z=z, alone_enc=alone_enc, alone_dec=alone_dec)


def _batch(pool, B):
    """B distinct cubes: the probes pool[0], pool[1], pool[2] in slots 0, B / 2, B - 1, fillers pool[3:] everywhere else."""
    x = pool[3:3 + B].clone()
    x[0], x[B // 2], x[B - 1] = pool[0], pool[1], pool[2]
    return x


@pytest.mark.parametrize("B", ENCODER_B)
def test_hyper_encoder_slots_equal_the_cube_alone(hyper, B):
    z = hyper["enc"](_batch(hyper["y"], B))
    assert float(z.abs().max()) > 0
    for slot, alone in zip((0, B // 2, B - 1), hyper["alone_enc"]):
        assert torch.equal(z[slot:slot + 1], alone), "hyper encoder B=%d: slot %d differs from the same cube at B=1 in %d of %d values" % (
            B, slot, int((z[slot:slot + 1] != alone).sum()), alone.numel())


@pytest.mark.parametrize("B", DECODER_B)
def test_hyper_decoder_slots_equal_the_cube_alone(hyper, B):
    loc, scale = hyper["dec"](_batch(hyper["z"], B), lower_bound=LOWER_BOUND)
    assert float(loc.abs().max()) > 0 and float(scale.max()) > LOWER_BOUND
    for slot, (loc1, scale1) in zip((0, B // 2, B - 1), hyper["alone_dec"]):
        for name, got, alone in (("loc", loc, loc1), ("scale", scale, scale1)):
            assert torch.equal(got[slot:slot + 1], alone), "hyper decoder B=%d %s: slot %d differs from the same cube at B=1 in %d of %d values" % (
                B, name, slot, int((got[slot:slot + 1] != alone).sum()), alone.numel())


def _held(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err, bound = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()), ATOL * max(1.0, float(np.abs(ref).max()))
    print("%s: largest error %.3g, bound %.3g (max|ref| %.3g)" % (what, err, bound, float(np.abs(ref).max())))
    assert err <= bound, "%s: max|diff| %.3g > %.3g" % (what, err, bound)


def test_the_cubes_alone_match_the_oracle(hyper):
    """What the slots are compared with is itself right: the B = 1 results against oracle.nets on the same weights (the
    oracle's convolutions are float32 on the CPU and take no other type)."""
    y, z = hyper["y"][:3].cpu().numpy(), hyper["z"][:3].cpu().numpy()
    z_ref = onets.hyper_encoder(onets.sub(hyper["w"], "hyper_encoder"), y)
    loc_ref, scale_ref = onets.hyper_decoder(onets.sub(hyper["w"], "hyper_decoder"), z)
    for i in range(3):
        _held(hyper["alone_enc"][i], z_ref[i:i + 1], "hyper encoder, probe %d at B=1" % i)
        _held(hyper["alone_dec"][i][0], loc_ref[i:i + 1], "hyper decoder loc, probe %d at B=1" % i)
        _held(hyper["alone_dec"][i][1], np.maximum(scale_ref[i:i + 1], LOWER_BOUND), "hyper decoder scale, probe %d at B=1" % i)


# ----------------------------------------------------------------------------------------------------------------------
# conv8_row_kernel<16,8> with the batch whole: pcgc_conv3d_bwd_data of an 8 -> 16 layer at 8^3
# ----------------------------------------------------------------------------------------------------------------------
def _bwd_data(dz, kernel):
    """dx [B,8,8,8,8] of the layer 8 -> 16, 3x3x3, stride 1, from dz [B,8,8,8,16]."""
    lib, B = _lib.hip(), int(dz.shape[0])
    nbytes = int(lib.pcgc_conv3d_bwd_workspace_bytes(8, 16, 3))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dx = torch.full((B, 8, 8, 8, 8), 7.0, device="cuda")
    _lib.check(lib.pcgc_conv3d_bwd_data(_lib.dptr(dz), _lib.dptr(kernel), _lib.dptr(dx), B, 8, 8, 16, 3, 1, 0, _lib.dptr(ws), nbytes,
                                        _lib.stream()), "pcgc_conv3d_bwd_data")
    return dx


@pytest.fixture(scope="module")
def layer():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(59)
    kernel = torch.randn((3, 3, 3, 8, 16), generator=g) * (2.0 / (27 * 8)) ** 0.5
    dz = torch.randn((max(BWD_B) + 3, 8, 8, 8, 16), generator=g)
    kd, dzd = kernel.cuda(), dz.cuda()
    alone = [_bwd_data(dzd[i:i + 1].contiguous(), kd) for i in range(3)]
    return dict(kernel=kernel, dz=dzd, kd=kd, alone=alone)


@pytest.mark.parametrize("B", BWD_B)
def test_bwd_data_of_the_8_to_16_layer_slots_equal_the_cube_alone(layer, B):
    dx = _bwd_data(_batch(layer["dz"], B), layer["kd"])
    assert float(dx.abs().max()) > 0
    for slot, alone in zip((0, B // 2, B - 1), layer["alone"]):
        assert torch.equal(dx[slot:slot + 1], alone), "bwd-data 8->16 B=%d: slot %d differs from the same cube at B=1 in %d of %d values" % (
            B, slot, int((dx[slot:slot + 1] != alone).sum()), alone.numel())


def test_bwd_data_of_the_8_to_16_layer_alone_matches_the_oracle(layer):
    """The gradient w.r.t. the input of a stride-1 'same' convolution is the 'same' convolution of dz with the filter flipped
    in space and its channel axes swapped: oracle.nets.conv3d_same on that filter (float32 on the CPU)."""
    flipped = layer["kernel"].flip(0, 1, 2).permute(0, 1, 2, 4, 3).contiguous().numpy()
    ref = onets.conv3d_same(layer["dz"][:3].cpu().numpy(), flipped)
    for i in range(3):
        _held(layer["alone"][i], ref[i:i + 1], "bwd-data 8->16 at 8^3, probe %d at B=1" % i)
