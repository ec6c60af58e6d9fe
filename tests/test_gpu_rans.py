"""Colour stream version 2 on the device: the rANS kernels (csrc/rans.hip) byte for byte against the numpy statement of the rule
(tests/_rans_ref.py), the whole codec with coder="rans" against tests/_raht_ref.py and the reference's pack_v2, its rate against the
reference's empirical entropy, and the command line (compress --color_coder rans)."""
import functools
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raht_ref as ref                                                  # noqa: E402
import _rans_ref as rans                                                 # noqa: E402
from test_gpu_colorcodec import CASES, STEPS, _coloured_cloud            # noqa: E402
from test_rans_host import ALPHABETS, sizes_for                          # noqa: E402
from pcgcv1_amd import _lib                                              # noqa: E402
from pcgcv1_amd import colorcodec as cc                                  # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

# profiles/colorcodec_rans_rd.txt, "test cloud": the largest measured version 2 bits / H of the six steps is 1.1370 (step 32), so
# m2 = 1.1370 - 1 + 0.05
RATE_MARGIN_RANS = 0.1870


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def test_format_constants_are_defined_twice_and_agree():
    assert (cc.RANS_STEPS, cc.RANS_MIN_SYMBOLS, cc.RANS_LOW, cc.RANS_LANES) == (rans.S, rans.T, rans.L, rans.LANES)


@pytest.mark.parametrize("steps", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(ALPHABETS))
def test_kernels_give_the_references_bytes(name, steps):
    """idle lanes (n < 64), the 64 / 65 boundary, a one-symbol last chunk, several chunks, the largest LDS table"""
    cdf, draw = ALPHABETS[name]
    rng = np.random.default_rng(100 + steps)
    for n in sizes_for(steps):
        sym = draw(rng, n)
        want, want_sizes = rans.encode(sym, [n], [cdf], steps)
        got, sizes = cc.rans_encode(sym, [n], [cdf], steps)
        assert np.array_equal(sizes, want_sizes), (name, steps, n, sizes, want_sizes)
        assert got == want, (name, steps, n)
        back, status = cc.rans_decode(got, sizes, [n], [cdf], steps)
        assert status.shape == (len(sizes),) and not status.any(), (name, steps, n, status)
        assert back.dtype == np.int16 and np.array_equal(back, sym), (name, steps, n)


def test_levels_alternating_between_one_chunk_and_several():
    names = ["two_symbols", "amax2047_escapes", "amax3_ratio1", "nearly_flat", "amax2047_escapes", "two_symbols"]
    steps = 2
    counts = [96, 3 * 128 + 3, 3, 3 * 100, 126, 129 * 3]                  # chunks: 1, 4, 1, 3, 1, 4; an empty level in between below
    rng = np.random.default_rng(7)
    counts.insert(3, 0)
    names.insert(3, "two_symbols")
    cdfs = [ALPHABETS[k][0] for k in names]
    sym = np.concatenate([ALPHABETS[k][1](rng, n) for k, n in zip(names, counts)])
    want, want_sizes = rans.encode(sym, counts, cdfs, steps)
    assert len(want_sizes) == 1 + 4 + 1 + 0 + 3 + 1 + 4
    got, sizes = cc.rans_encode(sym, counts, cdfs, steps)
    assert np.array_equal(sizes, want_sizes) and got == want
    back, status = cc.rans_decode(got, sizes, counts, cdfs, steps)
    assert not status.any() and np.array_equal(back, sym)
    with pytest.raises(ValueError, match="alphabet"):
        cc.rans_encode(np.array([0, 1, 2], np.int16), [3], [ALPHABETS["two_symbols"][0]], 1)
    with pytest.raises(ValueError, match="chunk sizes"):
        cc.rans_decode(got, sizes[:-1], counts, cdfs, steps)
    with pytest.raises(ValueError, match="chunk sizes"):
        cc.rans_decode(got + b"\0", np.concatenate([sizes[:-1], sizes[-1:] + 1]), counts, cdfs, steps)


@functools.lru_cache(maxsize=None)
def _reference(name, step):
    """the numpy rule's decoded colours and what it hands to the container: computed once per (case, step)"""
    p, c = CASES[name] if name in CASES else _coloured_cloud()
    want, q, sub, _ = ref.codec(p, c, step)
    d = ref.depth_of(p)
    counts = np.bincount(sub, minlength=3 * d + 1)
    qg = q[ref.subband_order(sub)]
    n_coded = cc.coded_levels(counts)
    k = int(counts[:n_coded].sum())
    lev = np.repeat(np.arange(n_coded), counts[:n_coded])
    biggest = np.zeros(n_coded, np.int64)
    np.maximum.at(biggest, lev, np.abs(qg[:k]).max(1))
    amax = np.minimum(biggest, cc.AMAX_CAP).astype(np.int32)
    a = amax[lev][:, None]
    inside = np.abs(qg[:k]) <= a
    sym = np.where(inside, qg[:k] + a, 2 * a + 1).astype(np.int16)
    pos = np.flatnonzero(~inside.reshape(-1))
    data = rans.pack_v2(d, len(p), step, counts, amax, sym, qg[k:], pos, qg[:k].reshape(-1)[pos])
    return want, data, ref.empirical_bits(q, sub), counts


@pytest.mark.parametrize("name", sorted(CASES))
def test_codec_v2_is_the_reference_bit_for_bit(name):
    p, c = CASES[name]
    for step in STEPS:
        want, want_data, _, counts = _reference(name, step)
        data = cc.encode_colors(p, c, step, coder="rans")
        assert data[4] == 2 and data == want_data, (name, step, len(data), len(want_data))
        got = cc.decode_colors(p, data)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, step, int((got != want).any(1).sum()))
        v1 = cc.encode_colors(p, c, step)
        assert v1[4] == 1 and v1 == cc.encode_colors(p, c, step, coder="range")          # the default is version 1, untouched
        n_coded = struct.unpack("<H", data[6:8])[0]
        assert n_coded == struct.unpack("<H", v1[6:8])[0]
        for l in range(n_coded):                                             # the same (amax, ratios) as version 1 for the same input
            assert struct.unpack("<HHHH", data[36 + 14 * l:44 + 14 * l]) == struct.unpack("<HHHH", v1[36 + 12 * l:44 + 12 * l]), (name, step, l)
        assert cc.encode_colors(p, c, step, coder="rans") == data           # the same bytes again
        shuffle = np.random.default_rng(step).permutation(len(p))
        assert cc.encode_colors(p[shuffle], c[shuffle], step, coder="rans") == data       # the file does not depend on the row order
        assert np.array_equal(cc.decode_colors(p[shuffle], data), want[shuffle])
    if name == "shell_res256":
        assert 1 in cc.level_coders(counts) and 0 in cc.level_coders(counts)


def test_v2_refusals_are_version_1s():
    """both are rejected on the host, before any kernel runs"""
    p, c = CASES["shell_res256"]
    data = cc.encode_colors(p, c, 4, coder="rans")
    other, _ = CASES["dense_res20"]
    with pytest.raises(ValueError, match="other geometry"):
        cc.decode_colors(other, data)
    with pytest.raises(ValueError, match="truncated"):
        cc.decode_colors(p, data[:len(data) // 2])
    with pytest.raises(ValueError, match="version 3, this decoder reads version 1"):
        cc.decode_colors(p, data[:4] + b"\x03" + data[5:])
    with pytest.raises(ValueError, match="coder"):
        cc.encode_colors(p, c, 4, coder="huffman")


def test_rate_v2_against_the_references_empirical_entropy():
    """bits <= (1 + m2) H + 8 header bytes at all six steps (H per point is at most 16.4 < 24, profiles/colorcodec_rd.txt); H is the
    numpy reference's, m2 = RATE_MARGIN_RANS comes from profiles/colorcodec_rans_rd.txt"""
    p, c = _coloured_cloud()
    for step in STEPS:
        _, want_data, h, _ = _reference("coloured_cloud", step)
        assert h < 24 * len(p)
        data = cc.encode_colors(p, c, step, coder="rans")
        bits, head = 8 * len(data), cc.header_bytes(data)
        print("step", step, "bits", bits, "H", h, "bits / H", bits / h, "header bytes", head, "bpp", bits / len(p))
        assert data == want_data
        assert bits <= (1 + RATE_MARGIN_RANS) * h + 8 * head, (step, bits, h, bits / h)


def test_cli_color_coder_rans(tmp_path, monkeypatch):
    from pcgcv1_amd import test as cli
    pts, col = _coloured_cloud()
    ply = tmp_path / "col_vox7.ply"
    iop.write_ply_colors(str(ply), pts, col)
    monkeypatch.chdir(tmp_path)
    five = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
    common = ["--ckpt_dir=synthetic:7:sparse", "--min_num=20"]
    cli.main(["compress", str(ply), "v1"] + common + ["--colors", "raht", "--color_coder", "range"])
    cli.main(["compress", str(ply), "v2"] + common + ["--colors", "raht", "--color_coder", "rans"])
    for k in five:
        assert (tmp_path / "compressed" / ("v1." + k)).read_bytes() == (tmp_path / "compressed" / ("v2." + k)).read_bytes(), k
    assert (tmp_path / "compressed" / "v1.colors").read_bytes()[4] == 1
    assert (tmp_path / "compressed" / "v2.colors").read_bytes()[4] == 2
    cli.main(["decompress", "compressed/v1", "v1_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    cli.main(["decompress", "compressed/v2", "v2_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    lines1 = (tmp_path / "v1_rec.ply").read_text().splitlines()
    lines2 = (tmp_path / "v2_rec.ply").read_text().splitlines()
    assert len(lines1) > 1000 and lines1 == lines2
    assert iop.load_ply_colors(str(tmp_path / "v2_rec.ply"))[1] is not None
    with pytest.raises(SystemExit, match="color_coder"):
        cli.main(["compress", str(ply), "x"] + common + ["--color_coder", "rans"])
