"""The scan smoothing on the device (csrc/smooth.hip: pcgc_smooth_step; pcgcv1_amd/smooth.py) against the rule in numpy
(tests/_smooth_ref.py): K, S, Q, moved and the output bits of one step, the chained passes, what the stage is for, and the
stage through voxelize_scan, register_scans and the three command lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _register_ref as rr                                               # noqa: E402
import _smooth_ref as ref                                                # noqa: E402
from pcgcv1_amd import _lib, ingest, register, smooth                    # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

CANARY = 0xA5
PAD = 8                                                                 # rows behind every output that must stay as they were


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


# ---------------------------------------------------------------------------- one step, called as the C ABI has it
class Call(object):
    """pcgc_smooth_step on canary-filled outputs with PAD rows to spare; the arrays come back in the order they went in"""

    def __init__(self, g, cells, radius, kmin, debug=True, ws=None):
        dev = torch.device("cuda")
        lib = _lib.hip()
        self.n = n = len(g)
        self.g_d = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(dev)
        self.out = torch.full(((n + PAD) * 3 * 4,), CANARY, dtype=torch.uint8, device=dev)
        self.moved = torch.full((n + PAD,), CANARY, dtype=torch.uint8, device=dev)
        self.K = torch.full(((n + PAD) * 4,), CANARY, dtype=torch.uint8, device=dev) if debug else None
        self.S = torch.full(((n + PAD) * 3 * 8,), CANARY, dtype=torch.uint8, device=dev) if debug else None
        self.Q = torch.full(((n + PAD) * 6 * 8,), CANARY, dtype=torch.uint8, device=dev) if debug else None
        self.ws = ws if ws is not None else torch.empty(int(lib.pcgc_smooth_workspace_bytes(cells[4], n)), dtype=torch.uint8, device=dev)
        self.rc = lib.pcgc_smooth_step(_lib.dptr(self.g_d), n, *cells, float(radius), int(kmin), _lib.dptr(self.out), _lib.dptr(self.moved),
                                       _lib.dptr(self.K), _lib.dptr(self.S), _lib.dptr(self.Q), _lib.dptr(self.ws), self.ws.numel(), _lib.stream())
        torch.cuda.synchronize()

    def arrays(self):
        """-> (out float32 [n,3], moved uint8 [n], K, S, Q or None), after checking that nothing behind row n was written"""
        got = []
        for t, dtype, width in ((self.out, np.float32, 3), (self.moved, np.uint8, 1), (self.K, np.int32, 1), (self.S, np.int64, 3),
                                (self.Q, np.int64, 6)):
            if t is None:
                got.append(None)
                continue
            raw = t.cpu().numpy()
            row = np.dtype(dtype).itemsize * width
            assert (raw[self.n * row:] == CANARY).all(), "wrote behind the last row"
            a = raw[:self.n * row].view(dtype)
            got.append(a.reshape(self.n, width) if width > 1 else a.copy())
        return got


def _cells(g, radius):
    g64 = np.asarray(g, np.float32).astype(np.float64)
    return register.cells_from_bounds(g64.min(0), g64.max(0), radius, "smooth")


def _against_the_rule(g, radius, kmin, debug=True, cells=None):
    """the step on g sorted by cell, against the reference on g as it came -> the reference's arrays"""
    g = np.ascontiguousarray(g, np.float32)
    cells = _cells(g, radius) if cells is None else cells
    order = register.cell_order(torch.from_numpy(g), cells).numpy()
    call = Call(g[order], cells, radius, kmin, debug)
    assert call.rc == 0, _lib.hip().pcgc_last_error().decode()
    out, moved, K, S, Q = call.arrays()
    want = ref.step(g, radius, kmin)
    assert np.array_equal(moved, want[1][order])
    assert out.view(np.uint32).tobytes() == want[0][order].view(np.uint32).tobytes()
    if debug:
        assert np.array_equal(K, want[2][order]) and np.array_equal(S, want[3][order]) and np.array_equal(Q, want[4][order])
    else:
        assert K is None and S is None and Q is None
    return want


def _sheet(seed, n, extent, noise=0.3, offset=0.0):
    """n points of a tilted, curved sheet in a box of `extent`, with noise across it"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, extent, (n, 3)) + offset
    p[:, 2] = offset + 0.4 * extent + 0.2 * (p[:, 0] - offset) + 0.02 * (p[:, 1] - offset) ** 2 + noise * rng.normal(size=n)
    return p.astype(np.float32)


@pytest.mark.parametrize("debug", [True, False])
@pytest.mark.parametrize("n", [1, 2, 63, 65, 257])
def test_wave_and_block_edges(n, debug):
    want = _against_the_rule(_sheet(n, n, 6.0), 2.0, 3, debug)
    assert want[1].any() == (n >= 63)


def test_a_few_thousand_points_of_a_noisy_surface():
    a = rr.surface(21, 4000)[0] * 2.0
    g = (a + np.random.default_rng(22).normal(size=a.shape) * 0.4).astype(np.float32)
    want = _against_the_rule(g, 3.0, 6)
    assert want[1].mean() > 0.95 and want[2].max() > 40
    assert not np.array_equal(want[0], g)


def test_a_neighbour_at_exactly_r_and_one_a_float32_step_beyond():
    beyond = np.nextafter(np.float32(3.0), np.float32(4.0))
    g = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, -3], [beyond, 0, 0], [0, -beyond, 0], [0.5, 0.25, 0.125]], np.float32)
    want = _against_the_rule(g, 3.0, 3)
    assert want[2][0] == 5                                     # itself, the three at r, the one nearby; not the two beyond


def test_coincident_points_count_each_and_a_cloud_of_one_place_stays():
    g = np.repeat(_sheet(5, 40, 5.0), 3, axis=0)
    want = _against_the_rule(g, 2.0, 6)
    assert (want[2] % 3 == 0).all() and want[1].any()
    same = np.tile(np.array([[1.5, -2.25, 7.0]], np.float32), (70, 1))
    want = _against_the_rule(same, 1.0, 3)
    assert (want[2] == 70).all() and want[1].all() and want[0].tobytes() == same.tobytes()      # C = 0: t = 0


def test_kmin_is_the_first_count_that_moves():
    g = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.5]], np.float32)
    want = _against_the_rule(g, 1.5, 5)                        # K = 4, 4, 4, 4, 5
    assert want[1].tolist() == [0, 0, 0, 0, 1] and want[0][4].tolist() == [0.0, 0.0, float(np.float32(0.5 + (-4 * 32768 / 5.0) / 65536.0))]
    assert _against_the_rule(g, 1.5, 4)[1].all()
    assert not _against_the_rule(g, 1.5, 6)[1].any()


def test_exactly_coplanar_and_collinear_neighbours():
    xy = np.stack(np.meshgrid(np.arange(9), np.arange(8), indexing="ij"), -1).reshape(-1, 2) * 0.75
    plane = np.concatenate([xy, np.full((len(xy), 1), 2.0)], 1).astype(np.float32)
    want = _against_the_rule(plane, 2.0, 3)
    assert want[1].all() and want[0].tobytes() == plane.tobytes()
    line = np.zeros((70, 3), np.float32)
    line[:, 0] = np.arange(70) * 0.5
    want = _against_the_rule(line, 2.0, 3)
    assert want[1].all() and want[0].tobytes() == line.tobytes()
    _against_the_rule(line @ np.array([[0.6, 0.8, 0], [-0.8, 0.6, 0], [0, 0, 1]], np.float32) + np.float32(0.3), 2.0, 3)       # a line askew


def test_cells_of_edge_two_and_a_negative_origin():
    g = _sheet(8, 500, 11.0, offset=-7.0)
    cells = _cells(g, 1.5)
    assert cells[0] == 2.0 and min(cells[1:4]) < 0
    assert _against_the_rule(g, 1.5, 4, cells=cells)[1].any()


def test_the_largest_radius():
    g = _sheet(9, 300, 60.0, noise=2.0)
    cells = _cells(g, 16.0)
    assert cells[0] == 16.0
    assert _against_the_rule(g, 16.0, 6, cells=cells)[2].max() > 20


def test_cells_wider_than_the_radius_need():
    g = _sheet(10, 200, 6.0)
    _against_the_rule(g, 1.25, 3, cells=(4.0, -1, -1, -1, 5))


def test_two_runs_give_the_same_bytes():
    g = _sheet(12, 3000, 30.0)
    cells = _cells(g, 3.0)
    g = g[register.cell_order(torch.from_numpy(g), cells).numpy()]
    a, b = Call(g, cells, 3.0, 6).arrays(), Call(g, cells, 3.0, 6).arrays()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_bad_input_raises_the_flag_and_the_next_call_clears_it():
    g = _sheet(13, 400, 10.0)
    cells = _cells(g, 2.0)
    order = register.cell_order(torch.from_numpy(g), cells).numpy()
    good = g[order]
    ws = Call(good, cells, 2.0, 4).ws
    want = ref.step(good, 2.0, 4)
    nan = good.copy()
    nan[123, 1] = np.nan
    outside = good.copy()
    outside[7] = good.max(0) + 100.0
    for bad in (good[::-1].copy(), nan, outside):
        call = Call(bad, cells, 2.0, 4, ws=ws)
        assert call.rc == 0 and (call.arrays()[1] == smooth.BAD_INPUT).all()
        with pytest.raises(RuntimeError, match="not finite or leaves the cells, or the points are not sorted"):
            smooth.smooth_step(torch.from_numpy(bad).cuda(), cells, 2.0, 4)
        again = Call(good, cells, 2.0, 4, ws=ws)
        out, moved, K, S, Q = again.arrays()
        assert again.rc == 0 and out.tobytes() == want[0].tobytes() and np.array_equal(moved, want[1]) and np.array_equal(K, want[2])


def test_every_bad_argument_is_refused():
    lib = _lib.hip()
    dev = torch.device("cuda")
    n = 10
    g = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    out, moved = torch.zeros_like(g), torch.zeros(n, dtype=torch.uint8, device=dev)
    K, S, Q = (torch.zeros(n * w, dtype=t, device=dev) for w, t in ((1, torch.int32), (3, torch.int64), (6, torch.int64)))
    ws = torch.empty(int(lib.pcgc_smooth_workspace_bytes(4, n)), dtype=torch.uint8, device=dev)
    good = dict(points=g, n=n, h=2.0, ox=0, oy=0, oz=0, res=4, radius=1.5, kmin=6, out=out, moved=moved, K=K, S=S, Q=Q, ws=ws,
                ws_bytes=ws.numel())

    def call(**change):
        a = dict(good, **change)
        return lib.pcgc_smooth_step(_lib.dptr(a["points"]), a["n"], a["h"], a["ox"], a["oy"], a["oz"], a["res"], a["radius"], a["kmin"],
                                    _lib.dptr(a["out"]), _lib.dptr(a["moved"]), _lib.dptr(a["K"]), _lib.dptr(a["S"]), _lib.dptr(a["Q"]),
                                    _lib.dptr(a["ws"]), a["ws_bytes"], _lib.stream())

    assert call() == 0 and call(K=None, S=None, Q=None) == 0
    torch.cuda.synchronize()
    for change in (dict(points=None), dict(out=None), dict(moved=None), dict(ws=None), dict(out=g), dict(n=0), dict(n=-1), dict(n=2 ** 31),
                   dict(res=0), dict(res=1025), dict(h=3.0), dict(h=0.5), dict(h=float("nan")), dict(ox=2 ** 29), dict(radius=0.0),
                   dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=2.5), dict(radius=16.5, h=32.0),
                   dict(kmin=2), dict(kmin=(1 << 22) + 1), dict(K=None), dict(S=None), dict(Q=None), dict(K=None, S=None),
                   dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0)):
        assert call(**change) != 0, change
        assert lib.pcgc_last_error().decode().startswith("pcgc_smooth_step: "), change
    assert call(radius=16.0, h=16.0) == 0                      # the largest radius there is
    torch.cuda.synchronize()
    for res, m in ((0, 10), (1025, 10), (4, 0), (4, -3), (4, 2 ** 31)):
        assert lib.pcgc_smooth_workspace_bytes(res, m) == 0
    assert lib.pcgc_smooth_workspace_bytes(4, 10) == lib.pcgc_feature_workspace_bytes(4, 10) > 0


# ---------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("iters", [1, 2])
def test_the_passes_equal_the_chain_of_the_rule_in_the_callers_order(iters):
    a = rr.surface(31, 3000)[0] * 2.0
    rng = np.random.default_rng(32)
    g = (a + rng.normal(size=a.shape) * 0.4).astype(np.float32)
    g = np.concatenate([g, np.array([[90.0, 90.0, 90.0]], np.float32)])[rng.permutation(len(g) + 1)]            # and a stray
    got, moved = smooth.smooth_grid(g, 3.0, iters, 6)
    want, want_moved = ref.chain(g, 3.0, iters, 6)
    assert got.dtype == np.float32 and got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert np.array_equal(moved, want_moved) and moved.sum() == len(g) - 1
    stray = int(np.nonzero(~moved)[0][0])
    assert g[stray].tolist() == [90.0, 90.0, 90.0] and got[stray].tobytes() == g[stray].tobytes()


def test_smooth_grid_refuses_what_is_not_finite_and_takes_nothing():
    with pytest.raises(ValueError, match="finite"):
        smooth.smooth_grid(np.array([[0, 0, np.nan]], np.float32), 3.0)
    with pytest.raises(ValueError, match="^smooth: "):
        smooth.smooth_grid(np.zeros((4, 3), np.float32), 3.0, iters=9)
    out, moved = smooth.smooth_grid(np.zeros((0, 3), np.float32), 3.0)
    assert out.shape == (0, 3) and moved.shape == (0,)


# ---------------------------------------------------------------------------- what it is for
SCALE, PER_SCAN, SIGMA, BITS = 4.0, 15000, 0.5, 9


@pytest.fixture(scope="module")
def noisy():
    """Two independent samplings of _register_ref's bumpy ellipsoid at 4 voxels per unit (radii about 40, 34 and 28 voxels),
    15 000 points each, merged; noise of 0.5 voxel per axis.  Everything is measured on one frame of 1 voxel per unit."""
    from scipy.spatial import cKDTree
    clean = np.concatenate([rr.surface(11, PER_SCAN)[0], rr.surface(12, PER_SCAN)[0]]) * SCALE
    raw = clean + np.random.default_rng(5).normal(size=clean.shape) * SIGMA
    frame = ingest.Frame(np.floor(raw.min(0)) - 4.0, 1.0, BITS)
    tree = cKDTree(rr.surface(13, 200000)[0] * SCALE)
    thinned = ref.scan(raw, frame.origin, frame.step, 3.0, 2, 6)[0]
    thinned_clean = ref.scan(clean, frame.origin, frame.step, 3.0, 2, 6)[0]
    return {"clean": clean, "raw": raw, "frame": frame, "tree": tree, "thinned": thinned, "thinned_clean": thinned_clean}


def test_the_shell_of_a_noisy_scan_gets_one_voxel_thick(noisy):
    """The reference's figures, computed on the CPU before this test was written:
        noise-free union   13 623 voxels, RMS to the dense sampling 0.150 voxel (the sampling's own floor)
        raw, sigma = 0.5   19 139 voxels = 1.405 x, RMS 0.522
        after 3:2          13 486 voxels = 0.990 x, RMS 0.212 = 0.406 of the raw cloud's
        noise-free at 3:2  13 512 voxels: 0.81 % fewer, RMS 0.213
    The thresholds are the issue's; the device must then give the reference's voxels exactly."""
    f = noisy["frame"]

    def count(p):
        return ref.voxels(p, f.origin, f.step, f.bits)

    base, raw, thin, thin_clean = count(noisy["clean"]), count(noisy["raw"]), count(noisy["thinned"]), count(noisy["thinned_clean"])
    rms_raw, rms_thin = ref.rms_to(noisy["raw"], noisy["tree"]), ref.rms_to(noisy["thinned"], noisy["tree"])
    print("voxels: noise-free %d, raw %d (%.3f x), thinned %d (%.3f x), noise-free thinned %d (%.2f %%); rms raw %.3f, thinned %.3f (%.3f)"
          % (base, raw, raw / base, thin, thin / base, thin_clean, 100.0 * abs(thin_clean - base) / base, rms_raw, rms_thin, rms_thin / rms_raw))
    assert raw >= 1.3 * base
    assert thin <= 1.05 * base
    assert rms_thin <= 0.6 * rms_raw
    assert abs(thin_clean - base) <= 0.02 * base
    got = ingest.voxelize_scan(noisy["raw"], frame=f, smooth="3:2")
    want = ingest.voxelize_scan(noisy["thinned"], frame=f)
    assert len(got[0]) == thin and np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    plain = ingest.voxelize_scan(noisy["raw"], frame=f)
    assert len(plain[0]) == raw


def test_smooth_scan_equals_the_rule_and_reports(noisy):
    f = noisy["frame"]
    raw = noisy["raw"].copy()
    raw[5] = (np.nan, 0.0, 0.0)
    raw[77, 2] = -np.inf
    got, report = smooth.smooth_scan(raw, f, "3:2")
    want, moved = ref.scan(raw, f.origin, f.step, 3.0, 2, 6)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert got[5].tobytes() == raw[5].tobytes() and got[77].tobytes() == raw[77].tobytes()
    assert report["spec"] == "3:2:6" and report["points"] == len(raw) - 2 and report["moved"] == int(moved.sum())
    d = (want[moved] - raw[moved]) / f.step
    assert abs(report["rms_move"] - float(np.sqrt((d * d).sum(1).mean()))) < 1e-4 and 0.2 < report["rms_move"] < 0.8


# ---------------------------------------------------------------------------- through the layers
UNIT, VOXEL = 0.01, 0.005                                    # scan units per unit of the surface; the voxel edge: 2 voxels per unit


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """two samplings of the surface in scanner units with colours, noise of 0.3 voxel, and one stray far from both (whole
    surfaces: point-to-point steps between two noisy halves slide along the overlap and do not end by the stopping rule)"""
    rng = np.random.default_rng(41)
    halves = []
    for seed in (42, 43):
        x = rr.surface(seed, 2500)[0]
        x = (x + rng.normal(size=x.shape) * 0.15) * UNIT
        halves.append((x, np.clip(np.rint(x / UNIT * 8.0), 0, 255).astype(np.uint8), None))
    stray = (rr.CENTRE + np.array([0.0, 0.0, 16.0])) * UNIT
    halves[0] = (np.concatenate([halves[0][0], stray[None]]), np.concatenate([halves[0][1], np.array([[1, 2, 3]], np.uint8)]), None)
    d = tmp_path_factory.mktemp("smooth")
    names = [str(d / ("half%d.ply" % k)) for k in range(2)]
    for name, (p, col, _) in zip(names, halves):
        iop.write_ply_colors(name, p, col)
    union = (np.concatenate([h[0] for h in halves]), np.concatenate([h[1] for h in halves]))
    iop.write_ply_colors(str(d / "union.ply"), *union)
    return {"dir": d, "halves": halves, "names": names, "union": union, "stray": len(halves[0][0]) - 1}


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        else:
            assert x == y


def test_voxelize_scan_with_smooth_is_voxelize_scan_of_smooth_scan(scan):
    p, col = scan["union"]
    raw_frame = ingest.fit_frame(p, voxel_size=VOXEL)
    smoothed, report = smooth.smooth_scan(p, raw_frame, "3:2")
    assert report["moved"] == len(p) - 1 and smoothed[scan["stray"]].tobytes() == p[scan["stray"]].tobytes()
    _same(ingest.voxelize_scan(p, col, voxel_size=VOXEL, smooth="3:2"), ingest.voxelize_scan(smoothed, col, voxel_size=VOXEL))
    _same(ingest.voxelize_scan(p, col, bits=7, smooth=smooth.parse_spec("3:2")),
          ingest.voxelize_scan(smooth.smooth_scan(p, ingest.fit_frame(p, bits=7), "3:2")[0], col, bits=7))
    _same(ingest.voxelize_scan_clean(p, col, voxel_size=VOXEL, clean="stat:20:2.0", smooth="3:2"),
          ingest.voxelize_scan_clean(smoothed, col, voxel_size=VOXEL, clean="stat:20:2.0"))
    # nothing asked, nothing changed
    _same(ingest.voxelize_scan(p, col, voxel_size=VOXEL, smooth=None), ingest.voxelize_scan(p, col, voxel_size=VOXEL))
    a, b = ingest.voxelize_scan_report(p, col, voxel_size=VOXEL, smooth=None), ingest.voxelize_scan_report(p, col, voxel_size=VOXEL)
    _same(a[0], b[0])
    assert a[1] is None and b[1] is None
    with pytest.raises(ValueError, match="^smooth: "):
        ingest.voxelize_scan(p, col, voxel_size=VOXEL, smooth="3:0")


def test_the_stray_is_left_by_the_smoothing_and_removed_by_the_cleaning(scan):
    p, col = scan["union"]
    plain = ingest.voxelize_scan(p, col, voxel_size=VOXEL, smooth="3:2")
    stray_voxel = np.floor((p[scan["stray"]] - plain[4].origin) / VOXEL + 0.5).astype(np.int32)
    assert (plain[0] == stray_voxel).all(1).any()              # where it was: the smoothing did not move it
    out, line = ingest.voxelize_scan_report(p, col, voxel_size=VOXEL, clean="stat:20:2.0", smooth="3:2")
    lines = line.split("\n")
    assert lines[0].startswith("smooth: 3:2:6 moved %d of %d points" % (len(p) - 1, len(p))) and lines[1].startswith("clean: stat:20:2.0 removed ")
    kept = ingest.apply_frame(out[0], out[4])
    assert np.abs(kept - p[scan["stray"]]).max(1).min() > 10 * VOXEL                  # and the cleaning dropped its voxel
    before, after = (int(v) for v in lines[0].split("voxels ")[-1].split(" -> "))
    assert after == len(plain[0]) and before > after


def test_the_ingest_command_line(scan, monkeypatch, capsys):
    monkeypatch.chdir(scan["dir"])
    p, col = scan["union"]
    ingest.main(["--input", "union.ply", "--output", "u.ply", "--voxel_size", repr(VOXEL), "--smooth", "3:2"])
    said = capsys.readouterr().out
    want, line = ingest.voxelize_scan_report(p, col, voxel_size=VOXEL, smooth="3:2")
    assert line.startswith("smooth: 3:2:6 moved ") and line in said and "clean:" not in said
    got_p, got_c = iop.load_ply_colors("u.ply")
    assert np.array_equal(got_p, want[0]) and np.array_equal(got_c, want[1]) and ingest.read_frame("u.frame") == want[4]
    ingest.main(["--input", "union.ply", "--output", "v.ply", "--voxel_size", repr(VOXEL)])
    said = capsys.readouterr().out
    plain = ingest.voxelize_scan(p, col, voxel_size=VOXEL)
    assert "smooth:" not in said and np.array_equal(iop.load_ply_colors("v.ply")[0], plain[0]) and len(plain[0]) > len(want[0])
    with pytest.raises(SystemExit):
        ingest.main(["--input", "missing.ply", "--output", "w.ply", "--bits", "7", "--smooth", "17"])              # before the file is read
    assert "smooth: the radius" in capsys.readouterr().err


def test_the_register_command_line(scan, monkeypatch, capsys):
    monkeypatch.chdir(scan["dir"])
    args = dict(voxel_size=VOXEL, metric="point", max_dist=(2.0,), tol=0.02, names=scan["names"])
    flags = ["--voxel_size", repr(VOXEL), "--metric", "point", "--max_dist", "2", "--tol", "0.02"]
    base = register.register_scans(scan["halves"], **args)
    none = register.register_scans(scan["halves"], smooth=None, **args)
    assert sorted(none) == sorted(base) == ["aligned", "merged", "poses"]
    _same(none["merged"], base["merged"])
    out = register.register_scans(scan["halves"], smooth="3:2", **args)
    assert out["smooth"].startswith("smooth: 3:2:6 moved ") and out["aligned"][0].tobytes() == base["aligned"][0].tobytes()
    _same(out["merged"], ingest.voxelize_scan(out["aligned"][0], out["aligned"][1], voxel_size=VOXEL, smooth="3:2"))
    assert len(out["merged"][0]) < len(base["merged"][0])
    register.main(["--input"] + scan["names"] + ["--output", "m.ply", "--smooth", "3:2"] + flags)
    said = capsys.readouterr().out
    assert out["smooth"] in said
    got_p, got_c = iop.load_ply_colors("m.ply")
    assert np.array_equal(got_p, out["merged"][0]) and np.array_equal(got_c, out["merged"][1])
    register.main(["--input"] + scan["names"] + ["--output", "m0.ply"] + flags)
    assert "smooth:" not in capsys.readouterr().out and np.array_equal(iop.load_ply_colors("m0.ply")[0], base["merged"][0])


def test_the_compress_command_line(scan, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    monkeypatch.chdir(scan["dir"])
    ckpt = "--ckpt_dir=synthetic:0"
    five = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
    ingest.main(["--input", "union.ply", "--output", "s7.ply", "--bits", "7", "--smooth", "3:2"])
    line = [x for x in capsys.readouterr().out.split("\n") if x.startswith("smooth: ")]
    assert len(line) == 1
    cli.main(["compress", "s7.ply", "a", ckpt])
    capsys.readouterr()
    cli.main(["compress", "union.ply", "b", ckpt, "--voxelize", "7", "--smooth", "3:2"])
    said = capsys.readouterr().out
    assert line[0] in said and "smooth=Spec(3:2:6)" in said
    assert all(open("compressed/a." + k, "rb").read() == open("compressed/b." + k, "rb").read() for k in five)
    assert open("compressed/b.frame", "rb").read() == open("s7.frame", "rb").read()
    cli.main(["compress", "union.ply", "c", ckpt, "--voxelize", "7"])
    said = capsys.readouterr().out
    assert "smooth:" not in said and "smooth=" not in said     # neither the line nor a word in the arguments it prints
    assert any(open("compressed/c." + k, "rb").read() != open("compressed/b." + k, "rb").read() for k in five)          # another cloud
    for argv in (["compress", "s7.ply", "d", ckpt, "--smooth", "3:2"], ["decompress", "compressed/b", "b.ply", ckpt, "--smooth", "3:2"],
                 ["compress", "union.ply", "d", ckpt, "--voxelize", "7", "--smooth", "3:2:1"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert "smooth" in capsys.readouterr().err
    assert not os.path.exists("compressed/d.strings")
