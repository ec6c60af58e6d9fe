"""The colour rate control on the device (csrc/color_rc.hip, colorcodec.encode_colors_target): the sweep and the six sums
integer for integer against numpy (tests/_color_rc_ref.py), the closed-loop probe byte for byte against a real encode and decode,
both targets' contracts, and the command line."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_rc_ref as rcref                                            # noqa: E402
from pcgcv1_amd import _lib, metrics, synthetic                          # noqa: E402
from pcgcv1_amd import colorcodec as cc                                  # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

GRID = [cc.grid_step(j) for j in range(cc.QSTEP_GRID_MIN, cc.QSTEP_GRID_MAX + 1)]
STEPS32 = GRID[:8] + GRID[8::3][:22] + [37.5, 100.0]                    # K = 32, 0.25 first
PROBE_STEPS = (0.25, 1, 4, 37.5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _dense(seed, res, n, keep):
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))][:keep]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def _twelve_bit():
    p, c = _dense(14, 4096, 3100, 3001)
    p[0] = [4095, 0, 4095]
    assert len(np.unique(p, axis=0)) == 3001
    return p, c


def _surface():
    """test_gpu_colorcodec.py's coloured cloud on one shell at res 140: a smooth colour field plus noise of sigma 10"""
    pts = synthetic.make_cloud(seed=5, res=140, n_shells=1, rmin=0.2, rmax=0.4).astype(np.int32)
    t = pts.astype(np.float64) / 140
    col = np.stack([128 + 100 * np.sin(7 * t[:, 0] + 3 * t[:, 1]), 128 + 100 * np.cos(5 * t[:, 1] - 2 * t[:, 2]), 255 * t[:, 2]], -1)
    col = np.clip(np.rint(col + np.random.default_rng(5).normal(0, 10, col.shape)), 0, 255).astype(np.uint8)
    return pts, col


def _cases():
    surface = _surface()
    return {
        "one_point": (np.array([[3, 4, 5]], np.int32), np.array([[7, 200, 9]], np.uint8)),
        "raw_only_48": _dense(1, 16, 400, 48),
        "first_coded_49": _dense(1, 16, 400, 49),
        "twelve_bit_3001": _twelve_bit(),
        "surface_20k": surface,
        "constant_colour": (surface[0][:5000], np.full((5000, 3), 93, np.uint8)),
    }


CASES = _cases()
_REF = {}


def _ref_sweep(name):
    """the numpy sweep of a case over STEPS32, computed once"""
    if name not in _REF:
        _REF[name] = rcref.sweep(*CASES[name], STEPS32)
    return _REF[name]


def _quantize_and_abs_sums(p, c, step):
    """the codec's own two kernels at one step -> (sums int64 [37, 3], max |q| int32 [37], level counts)"""
    import torch
    lib, s = _lib.hip(), _lib.stream()
    plan = cc.Plan(p)
    rgb = torch.from_numpy(np.ascontiguousarray(c)).to(plan.dev)
    attr = torch.empty((plan.m, 3), dtype=torch.float64, device=plan.dev)
    _lib.check(lib.pcgc_raht_load_colors(_lib.dptr(rgb), _lib.dptr(plan.point_of_leaf), plan.m, _lib.dptr(attr), s))
    plan.transform(attr)
    q = torch.empty((plan.m, 3), dtype=torch.int32, device=plan.dev)
    tops_d = torch.empty(64, dtype=torch.int32, device=plan.dev)
    _lib.check(lib.pcgc_raht_quantize(_lib.dptr(attr), _lib.dptr(plan.order), _lib.dptr(plan.subband), plan.m, float(step), _lib.dptr(q), _lib.dptr(tops_d), s))
    n_coded = cc.coded_levels(plan.level_counts)
    k_raw = int(plan.level_counts[:n_coded].sum())
    tops = tops_d.cpu().numpy()[:37]
    amax_d = torch.zeros(64, dtype=torch.int32, device=plan.dev)
    amax_d[:n_coded] = torch.from_numpy(np.minimum(tops[:n_coded], cc.AMAX_CAP).astype(np.int32)).to(plan.dev)
    sums_d = torch.empty(37 * 3, dtype=torch.int64, device=plan.dev)
    _lib.check(lib.pcgc_raht_abs_sums(_lib.dptr(q), _lib.dptr(plan.order), _lib.dptr(plan.subband), k_raw, _lib.dptr(amax_d), _lib.dptr(sums_d), s))
    tops = tops.copy()
    tops[n_coded:] = 0
    return sums_d.cpu().numpy().reshape(37, 3), tops, plan.level_counts


@pytest.mark.parametrize("name", sorted(CASES))
def test_rate_sweep_equals_the_numpy_reference(name):
    p, c = CASES[name]
    want_s, want_t = _ref_sweep(name)
    got_s, got_t = cc.rate_sweep(p, c, STEPS32)                           # K = 32
    assert got_s.dtype == np.int64 and got_s.shape == (32, 37, 3) and got_t.dtype == np.int32 and got_t.shape == (32, 37)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_t, want_t), name
    for k in (0, 13):                                                    # K = 1: steps 0.25 and one further up
        one_s, one_t = cc.rate_sweep(p, c, [STEPS32[k]])
        assert np.array_equal(one_s[0], want_s[k]) and np.array_equal(one_t[0], want_t[k]), (name, k)
    all_s, all_t = cc.rate_sweep(p, c, GRID)                              # 73 steps: three launches
    assert np.array_equal(all_s[:8], want_s[:8]) and np.array_equal(all_t[:8], want_t[:8]) and all_s.shape == (73, 37, 3)
    assert np.array_equal(all_s[72], rcref.sweep(p, c, [128.0])[0][0])
    for k in (0, 20):                                                    # the same row from the codec's own kernels
        sums, tops, counts = _quantize_and_abs_sums(p, c, STEPS32[k])
        assert np.array_equal(sums, want_s[k]) and np.array_equal(tops, want_t[k]), (name, k)
    n_coded = cc.coded_levels(counts)
    if name in ("one_point", "raw_only_48"):                             # nothing is coded: every sum is zero
        assert n_coded == 0 and not want_s.any() and not want_t.any()
    if name == "first_coded_49":
        assert n_coded >= 1 and 0 < counts[:n_coded].sum() <= 49 - 1 and want_s[0].any()
    if name == "twelve_bit_3001":
        assert len(counts) == 37 and len(p) % 64 != 0 and (counts[:n_coded] == 0).any()             # empty subbands among the coded ones
    if name == "surface_20k":
        assert 19000 < len(p) < 22000 and 3 * counts.max() >= cc.RANS_MIN_SYMBOLS
        assert STEPS32[0] == 0.25 and want_t[0].max() > cc.AMAX_CAP       # the cap of min(|q|, 2048) is exercised
    if name == "constant_colour":
        assert not want_s.any() and not want_t.any() and n_coded > 5     # every hi is 0


def test_rate_sweep_refuses_bad_steps_without_launching():
    import torch
    lib, s = _lib.hip(), _lib.stream()
    p, c = CASES["first_coded_49"]
    plan = cc.Plan(p)
    coef = torch.zeros((plan.m, 3), dtype=torch.float64, device=plan.dev)
    sums = torch.full((33 * 37 * 3,), -7, dtype=torch.int64, device=plan.dev)
    tops = torch.full((33 * 37,), -7, dtype=torch.int32, device=plan.dev)

    def call(steps, k=None):
        a = np.ascontiguousarray(steps, np.float64)
        return lib.pcgc_raht_rate_sweep(_lib.dptr(coef), _lib.dptr(plan.order), _lib.dptr(plan.subband), plan.m, plan.m - 1, _lib.nptr(a),
                                        len(a) if k is None else k, _lib.dptr(sums), _lib.dptr(tops), s)

    for steps, k in (([1.0], 0), ([1.0] * 33, None), ([0.0], None), ([1.0, -2.0], None), ([float("nan")], None), ([float("inf")], None)):
        assert call(steps, k) == -1 and b"pcgc_raht_rate_sweep" in lib.pcgc_last_error()
    torch.cuda.synchronize()
    assert bool((sums == -7).all()) and bool((tops == -7).all())          # not even zeroed
    assert call([1.0] * 32) == 0
    with pytest.raises(ValueError, match="positive"):
        cc.rate_sweep(p, c, [1.0, 0.0])
    with pytest.raises(ValueError, match="at least one"):
        cc.rate_sweep(p, c, [])


@pytest.mark.parametrize("coder", ("range", "rans"))
@pytest.mark.parametrize("name", ("twelve_bit_3001", "surface_20k"))
def test_probe_equals_encode_then_decode(name, coder):
    p, c = CASES[name]
    for step in PROBE_STEPS:
        want = cc.decode_colors(p, cc.encode_colors(p, c, step, coder=coder))
        got = cc.probe_colors(p, c, step)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, coder, step, int((got != want).any(1).sum()))


def test_requantize_refuses_aliasing():
    import torch
    lib = _lib.hip()
    dev = _lib.require_gpu()
    a = torch.zeros((10, 3), dtype=torch.float64, device=dev)
    assert lib.pcgc_raht_requantize(_lib.dptr(a), 10, 1.0, _lib.dptr(a), _lib.stream()) == -1
    assert lib.pcgc_raht_requantize(_lib.dptr(a), 6, 1.0, ctypes.c_void_p(a.data_ptr() + 5 * 24), _lib.stream()) == -1
    assert lib.pcgc_raht_requantize(_lib.dptr(a), 5, 1.0, ctypes.c_void_p(a.data_ptr() + 5 * 24), _lib.stream()) == 0
    assert lib.pcgc_raht_requantize(_lib.dptr(a), 5, 0.0, ctypes.c_void_p(a.data_ptr() + 5 * 24), _lib.stream()) == -1


def test_sse6_exact_and_its_luma_psnr():
    rng = np.random.default_rng(21)
    for m in (1, 65, 20000):
        a, b = rng.integers(0, 256, (m, 3)).astype(np.uint8), rng.integers(0, 256, (m, 3)).astype(np.uint8)
        got = cc.sse6(a, b)
        assert got.dtype == np.int64 and got.tolist() == rcref.sse6(a, b).tolist(), m
        assert cc.sse6(a, a).tolist() == [0] * 6
        assert cc.sse6(b, a).tolist() == got.tolist()
    zero, full = np.zeros((20000, 3), np.uint8), np.full((20000, 3), 255, np.uint8)
    assert cc.sse6(zero, full).tolist() == [20000 * 255 ** 2] * 6         # the largest term, every row
    mixed = full.copy()
    mixed[:, 1] = 0                                                       # dr dg and dg db as negative as they get
    assert cc.sse6(mixed, full - mixed).tolist() == rcref.sse6(mixed, full - mixed).tolist() and cc.sse6(mixed, full - mixed)[3] == -20000 * 255 ** 2
    p, c = CASES["surface_20k"]
    noisy = np.clip(c.astype(np.int32) + rng.integers(-9, 10, c.shape), 0, 255).astype(np.uint8)
    want = metrics.color_metrics(p, c, p, noisy)
    mse = cc.yuv_mse(cc.sse6(c, noisy), len(p))
    for i in range(3):
        assert abs(cc.psnr_of_mse(mse[i]) - want["c[%d],PSNR1" % i]) < 1e-9, (i, cc.psnr_of_mse(mse[i]), want["c[%d],PSNR1" % i])
    with pytest.raises(ValueError, match="uint8"):
        cc.sse6(c, noisy.astype(np.int32))


def _psnr_y(p, c, data):
    return cc.psnr_of_mse(cc.yuv_mse(cc.sse6(cc.decode_colors(p, data), c), len(p))[0])


def _header_step(data):
    return struct.unpack("<d", data[16:24])[0]


@pytest.mark.parametrize("target", (30, 36, 42))
def test_psnr_contract(target):
    p, c = CASES["surface_20k"]
    data, rep = cc.encode_colors_target(p, c, psnr=target)
    j = rep["j"]
    assert cc.QSTEP_GRID_MIN < j < cc.QSTEP_GRID_MAX                      # the three targets lie inside this cloud's range
    assert data == cc.encode_colors(p, c, cc.grid_step(j)) and _header_step(data) == rep["qstep"] == cc.grid_step(j)
    y = _psnr_y(p, c, data)
    print("target", target, "report", rep, "decoded", y)
    assert y >= target and rep["psnr_y"] == y
    assert _psnr_y(p, c, cc.encode_colors(p, c, cc.grid_step(j + 1))) < target
    assert rep["bytes"] == len(data) and rep["bpp"] == 8 * len(data) / len(p) and rep["real_encodes"] == 1
    assert 2 <= rep["probes"] <= 2 + 7                                   # both ends, then 72 notches halved to one
    assert "est_bytes" not in rep and "j_est" not in rep


def test_psnr_unreachable_target_raises():
    """200 dB on the 20 000-point cloud.  The finest step of the grid, 0.25, does not fall short of it: it decodes to the input's
    very colours (every coefficient is off by at most 0.125), an infinite PSNR.  What makes 200 dB unreachable is that no file of
    20 000 points has a finite PSNR above psnr_ceiling = 165.1 dB: the refusal names that, and a target at the ceiling itself is
    met, by a file without luma error."""
    p, c = CASES["surface_20k"]
    assert np.array_equal(cc.probe_colors(p, c, 0.25), c)
    with pytest.raises(ValueError, match="out of reach.*%.4f dB" % cc.psnr_ceiling(len(p))):
        cc.encode_colors_target(p, c, psnr=200)
    with pytest.raises(ValueError, match="out of reach"):
        cc.encode_colors_target(p, c, psnr=float("inf"))
    data, rep = cc.encode_colors_target(p, c, psnr=cc.psnr_ceiling(len(p)))
    print(rep)
    assert rep["psnr_y"] == _psnr_y(p, c, data) == float("inf")
    assert rep["j"] < cc.QSTEP_GRID_MAX and _psnr_y(p, c, cc.encode_colors(p, c, cc.grid_step(rep["j"] + 1))) < cc.psnr_ceiling(len(p))


def test_psnr_shortfall_names_the_best_reachable(monkeypatch):
    p, c = CASES["surface_20k"]
    monkeypatch.setattr(cc, "QSTEP_GRID_MIN", 16)                         # a grid whose finest step is 4: lossy
    best = _psnr_y(p, c, cc.encode_colors(p, c, 4.0))
    assert 40 < best < 60
    with pytest.raises(ValueError, match="out of reach.*dB") as e:
        cc.encode_colors_target(p, c, psnr=200)
    assert ("%.4f dB" % best) in str(e.value) and "step, 4," in str(e.value)
    data, rep = cc.encode_colors_target(p, c, psnr=best)                  # ... and exactly reachable: the finest notch itself
    assert rep["j"] == 16 and data == cc.encode_colors(p, c, 4.0)


def test_psnr_trivial_target():
    p, c = CASES["surface_20k"]
    data, rep = cc.encode_colors_target(p, c, psnr=0, coder="rans")
    assert rep["j"] == cc.QSTEP_GRID_MAX and rep["probes"] == 2 and data == cc.encode_colors(p, c, 128.0, coder="rans")
    assert rep["psnr_y"] == _psnr_y(p, c, data)


@pytest.mark.parametrize("coder", ("range", "rans"))
def test_bpp_contract(coder):
    p, c = CASES["surface_20k"]
    for step in (2, 8, 32):
        budget = len(cc.encode_colors(p, c, step, coder=coder)) + 1
        data, rep = cc.encode_colors_target(p, c, bpp=8 * budget / len(p), coder=coder)
        j = rep["j"]
        print(coder, "budget", budget, "report", rep)
        assert len(data) <= budget and data == cc.encode_colors(p, c, cc.grid_step(j), coder=coder)
        assert j > cc.QSTEP_GRID_MIN and len(cc.encode_colors(p, c, cc.grid_step(j - 1), coder=coder)) > budget
        assert rep["real_encodes"] >= 2 and rep["real_encodes"] == abs(rep["j_est"] - j) + (2 if rep["j_est"] >= j else 1)
        assert cc.grid_step(j) <= step                                    # step itself fits, so the chosen one is no coarser
        assert rep["bytes"] == len(data) and rep["bpp"] == 8 * len(data) / len(p) and rep["probes"] == 1
        assert rep["psnr_y"] == _psnr_y(p, c, data) and rep["est_bytes"] > 0 and _header_step(data) == rep["qstep"]


def test_bpp_out_of_reach_and_trivial():
    p, c = CASES["twelve_bit_3001"]
    with pytest.raises(ValueError, match="out of reach.*bytes"):
        cc.encode_colors_target(p, c, bpp=8 * 8 / len(p))
    data, rep = cc.encode_colors_target(p, c, bpp=1000.0)
    assert rep["j"] == rep["j_est"] == cc.QSTEP_GRID_MIN and rep["real_encodes"] == 1 and data == cc.encode_colors(p, c, 0.25)


def test_determinism():
    p, c = CASES["surface_20k"]
    for kw in ({"psnr": 36}, {"bpp": 2.0}, {"bpp": 2.0, "coder": "rans"}):
        first, again = cc.encode_colors_target(p, c, **kw), cc.encode_colors_target(p, c, **kw)
        assert first[0] == again[0] and first[1] == again[1], kw


@pytest.mark.parametrize("coder", ("range", "rans"))
def test_plain_encode_is_unchanged(coder):
    """encode_colors at a step is still the container of the codec's own quantiser, symbols and tables, put together from the
    public pieces"""
    p, c = CASES["surface_20k"]
    data = cc.encode_colors(p, c, 4.0, coder=coder)
    plan = cc.Plan(p)
    counts = [int(x) for x in plan.level_counts]
    n_coded = cc.coded_levels(counts)
    k_raw = sum(counts[:n_coded])
    coef = cc.raht_forward(p, cc.rgb_to_ycocg(c))[0]
    order = plan.order.cpu().numpy()
    q = np.rint(coef[order] / 4.0).astype(np.int64)
    tops = np.array([np.abs(q[sum(counts[:l]):sum(counts[:l + 1])]).max(initial=0) for l in range(n_coded)])
    assert tops.max() <= cc.AMAX_CAP                                      # no escapes at this step
    amax = tops.astype(np.int32)
    symbols = (q[:k_raw] + np.repeat(amax, counts[:n_coded])[:, None]).astype(np.int16)
    if coder == "range":
        assert data == cc.pack(plan.d, plan.m, 4.0, counts, amax, symbols, q[k_raw:])
        return
    from pcgcv1_amd import coder_ops
    kinds = cc.level_coders(counts)
    base = np.concatenate([[0], np.cumsum(counts[:n_coded])])
    ratios = [[cc.ratio_of_sum(int(np.abs(q[base[l]:base[l + 1], ch]).sum()), counts[l]) for ch in range(3)] for l in range(n_coded)]
    cdfs = [cc.build_tables(int(amax[l]), ratios[l]) for l in range(n_coded)]
    streams, sizes = [], []
    for l in range(n_coded):
        sym = symbols[base[l]:base[l + 1]]
        if kinds[l] == cc.CODER_RANS:
            payload, sz = cc.rans_encode(sym.reshape(-1), [sym.size], [cdfs[l]])
            streams.append(payload)
            sizes.append(sz)
        else:
            streams.append(coder_ops.range_encode(sym, cdfs[l][None]) if len(sym) else b"")
            sizes.append(np.zeros(0, np.int64))
    assert cc.CODER_RANS in kinds
    assert data == cc.assemble_v2(plan.d, plan.m, 4.0, counts, amax, ratios, streams, sizes, q[k_raw:])


def test_cli_color_target(tmp_path, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4).astype(np.int32)
    t = pts.astype(np.float64) / 128
    col = np.stack([128 + 100 * np.sin(7 * t[:, 0] + 3 * t[:, 1]), 128 + 100 * np.cos(5 * t[:, 1] - 2 * t[:, 2]), 255 * t[:, 2]], -1)
    col = np.clip(np.rint(col + np.random.default_rng(5).normal(0, 10, col.shape)), 0, 255).astype(np.uint8)
    ply = tmp_path / "col_vox7.ply"
    iop.write_ply_colors(str(ply), pts, col)
    monkeypatch.chdir(tmp_path)
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--colors", "raht", "--color_target", "psnr:36"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("colors raht, target psnr:36")]
    assert len(line) == 1 and "luma PSNR" in line[0] and "probes" in line[0] and "real encodes" in line[0] and "color_qstep" in line[0]
    data = (tmp_path / "compressed" / "col_vox7.colors").read_bytes()
    assert data[:4] == cc.MAGIC and data[4] == cc.VERSION
    step = _header_step(data)
    on_grid = [j for j in range(cc.QSTEP_GRID_MIN, cc.QSTEP_GRID_MAX + 1) if cc.grid_step(j) == step]
    assert len(on_grid) == 1 and ("grid notch %d)" % on_grid[0]) in line[0]
    cli.main(["decompress", "compressed/col_vox7", "colour_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    rec_p, rec_c = iop.load_ply_colors(str(tmp_path / "colour_rec.ply"))
    assert rec_c is not None and len(rec_p) > 1000 and np.array_equal(rec_c, cc.decode_colors(rec_p.astype(np.int32), data))
    # bits per INPUT point: the file fits the budget, the next finer notch does not
    cli.main(["compress", str(ply), "bpp", "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--colors", "raht", "--color_target", "bpp:1.5",
              "--color_coder", "rans"])
    data = (tmp_path / "compressed" / "bpp.colors").read_bytes()
    assert data[4] == cc.VERSION_RANS and 8 * len(data) / len(pts) <= 1.5 and _header_step(data) in GRID
