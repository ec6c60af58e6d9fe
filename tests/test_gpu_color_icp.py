"""Coloured ICP on the device (csrc/color_icp.hip: pcgc_color_gradient; csrc/offgrid.hip: pcgc_register_color_step;
pcgcv1_amd/register.py, metric="color") against the rule in numpy (tests/_color_icp_ref.py): the gradients bit for bit, one
step sum by sum, then the loop on the three fixtures, register_scans and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _color_icp_ref as ref                                             # noqa: E402
import _register_ref as rr                                               # noqa: E402
from pcgcv1_amd import _lib, ingest, register                            # noqa: E402

CANARY = 0xA5
PAD = 8                                                                 # rows behind every output that must stay as they were
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


# ---------------------------------------------------------------------------- kernel 1, called as the C ABI has it
class Call(object):
    """pcgc_color_gradient on canary-filled outputs with PAD rows to spare; the arrays come back in the order they went in"""

    def __init__(self, g, normals, Y, cells, radius, kmin, debug=True, ws=None):
        dev = torch.device("cuda")
        lib = _lib.hip()
        self.n = n = len(g)
        self.g_d = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(dev)
        self.n_d = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(dev)
        self.Y_d = torch.from_numpy(np.ascontiguousarray(Y, np.int32)).to(dev)
        self.grad = torch.full(((n + PAD) * 3 * 8,), CANARY, dtype=torch.uint8, device=dev)
        self.valid = torch.full((n + PAD,), CANARY, dtype=torch.uint8, device=dev)
        self.K = torch.full(((n + PAD) * 4,), CANARY, dtype=torch.uint8, device=dev) if debug else None
        self.Q = torch.full(((n + PAD) * 6 * 8,), CANARY, dtype=torch.uint8, device=dev) if debug else None
        self.B = torch.full(((n + PAD) * 3 * 8,), CANARY, dtype=torch.uint8, device=dev) if debug else None
        self.ws = ws if ws is not None else torch.empty(int(lib.pcgc_color_gradient_workspace_bytes(cells[4], n)), dtype=torch.uint8,
                                                        device=dev)
        self.rc = lib.pcgc_color_gradient(_lib.dptr(self.g_d), _lib.dptr(self.n_d), _lib.dptr(self.Y_d), n, *cells, float(radius), int(kmin),
                                          _lib.dptr(self.grad), _lib.dptr(self.valid), _lib.dptr(self.K), _lib.dptr(self.Q), _lib.dptr(self.B),
                                          _lib.dptr(self.ws), self.ws.numel(), _lib.stream())
        torch.cuda.synchronize()

    def arrays(self):
        """-> (grad float64 [n,3], valid uint8 [n], K, Q, B or None), after checking that nothing behind row n was written"""
        got = []
        for t, dtype, width in ((self.grad, np.float64, 3), (self.valid, np.uint8, 1), (self.K, np.int32, 1), (self.Q, np.int64, 6),
                                (self.B, np.int64, 3)):
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
    return register.cells_from_bounds(g64.min(0), g64.max(0), radius, "icp")


def _against_the_rule(g, normals, Y, radius, kmin, debug=True, cells=None):
    """the kernel on the cloud sorted by cell, against the reference on the cloud as it came -> the reference's arrays"""
    g, normals, Y = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(normals, np.float32), np.ascontiguousarray(Y, np.int32)
    cells = _cells(g, radius) if cells is None else cells
    order = register.cell_order(torch.from_numpy(g), cells).numpy()
    call = Call(g[order], normals[order], Y[order], cells, radius, kmin, debug)
    assert call.rc == 0, _lib.hip().pcgc_last_error().decode()
    grad, valid, K, Q, B = call.arrays()
    want = ref.gradient(g, normals, Y, radius, kmin)
    assert np.array_equal(valid, want[1][order])
    assert grad.view(np.uint64).tobytes() == want[0][order].view(np.uint64).tobytes()
    if debug:
        assert np.array_equal(K, want[2][order]) and np.array_equal(Q, want[3][order]) and np.array_equal(B, want[4][order])
    else:
        assert K is None and Q is None and B is None
    return want


def _sphere_target():
    d = ref.fixture("sphere")
    return d["target"], ref.unit_normals(d["target_normals"]), ref.intensity(d["target_colors"])


def _sheet(seed, n, extent, offset=0.0, noise=0.05):
    """n points of a tilted, curved sheet in a box of `extent`, their unit normals and a textured intensity"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, extent, (n, 3)) + offset
    p[:, 2] = offset + 0.4 * extent + 0.2 * (p[:, 0] - offset) + 0.02 * (p[:, 1] - offset) ** 2 + noise * rng.normal(size=n)
    nrm = np.stack([np.full(n, -0.2), -0.04 * (p[:, 1] - offset), np.ones(n)], 1)
    return p.astype(np.float32), ref.unit_normals(nrm), ref.intensity(ref.texture(p))


@pytest.mark.parametrize("debug", [True, False])
@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 4000])
def test_gradients_equal_the_rule_bit_for_bit(n, debug):
    """the n points of the sphere fixture's target nearest to its first: less than a wave, a wave and one, more than a
    workgroup, and the whole fixture"""
    g, nrm, Y = _sphere_target()
    near = np.argsort(np.linalg.norm(g.astype(np.float64) - g[0].astype(np.float64), axis=1), kind="stable")[:n]
    want = _against_the_rule(g[near], nrm[near], Y[near], 3.0, 6, debug)
    assert want[1].any() == (n >= 63)
    if n == 4000:
        assert want[1].mean() > 0.95 and want[2].max() > 20 and not want[1].all()


def test_a_neighbour_at_exactly_r_and_one_a_float32_step_beyond():
    beyond = np.nextafter(np.float32(3.0), np.float32(4.0))
    g = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [-3, 0, 0], [beyond, 0, 0], [0, -beyond, 0], [0.5, 0.25, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (7, 1))
    Y = np.array([100000, 400000, 250000, 50000, 2550000, 0, 130000], np.int32)
    want = _against_the_rule(g, nrm, Y, 3.0, 3)
    assert want[2][0] == 5 and want[1][0] == 1                 # itself, the three at r, the one nearby; not the two beyond
    far = ref.gradient(g[[0, 1, 2, 3, 6]], nrm[:5], Y[[0, 1, 2, 3, 6]], 3.0, 3)[0][0]
    assert want[0][0].tobytes() == far.tobytes()               # ... whose loud intensities leave no trace


def test_coincident_points_count_each():
    g, nrm, Y = _sheet(5, 40, 5.0)
    g, nrm = np.repeat(g, 3, axis=0), np.repeat(nrm, 3, axis=0)
    Y = np.clip(np.repeat(Y, 3) + np.tile(np.array([0, 7, -5], np.int32), 40), 0, ref.Y_MAX)          # one place, three intensities
    want = _against_the_rule(g, nrm, Y, 2.0, 6)
    assert (want[2] % 3 == 0).all() and want[1].any()
    same = np.tile(np.array([[1.5, -2.25, 7.0]], np.float32), (70, 1))
    want = _against_the_rule(same, np.tile(np.array([0, 1, 0], np.float32), (70, 1)), np.arange(70, dtype=np.int32) * 1000, 1.0, 3)
    assert (want[2] == 70).all() and not want[1].any()         # one place: no offsets, no determinant


def test_collinear_neighbours_a_zero_normal_and_kmin():
    line = np.zeros((70, 3), np.float32)
    line[:, 0] = np.arange(70) * 0.5
    up = np.tile(np.array([0, 0, 1], np.float32), (70, 1))
    assert not _against_the_rule(line, up, np.arange(70, dtype=np.int32) * 1000, 2.0, 3)[1].any()
    g = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
    nrm, Y = np.tile(np.array([0, 0, 1], np.float32), (5, 1)), np.array([1000, 3000, 500, 2000, 100], np.int32)
    assert _against_the_rule(g, nrm, Y, 1.25, 5)[1].tolist() == [1, 0, 0, 0, 0]          # K = 5, 2, 2, 2, 2
    assert not _against_the_rule(g, nrm, Y, 1.25, 6)[1].any()
    for bad in ([0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]):
        nb = nrm.copy()
        nb[0] = bad
        assert not _against_the_rule(g, nb, Y, 1.25, 5)[1].any()
    for axis in range(3):                                     # every choice of the tangent basis' axis, and its ties
        for nvec in ([1, 1, 1], [1, 2, 3], [3, 1, 2], [2, 3, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0, -1], [0, -1, 0], [-1, 0, 0]):
            sheet, _, Ys = _sheet(40 + axis, 80, 4.0)
            _against_the_rule(np.roll(sheet, axis, axis=1), ref.unit_normals(np.tile(np.roll(np.array(nvec, np.float64), axis), (80, 1))), Ys,
                              2.0, 4)


def test_cells_of_edge_two_and_a_negative_origin():
    g, nrm, Y = _sheet(8, 500, 11.0, offset=-7.0)
    cells = _cells(g, 1.5)
    assert cells[0] == 2.0 and min(cells[1:4]) < 0
    assert _against_the_rule(g, nrm, Y, 1.5, 4, cells=cells)[1].any()


def test_the_largest_radius():
    g, nrm, Y = _sheet(9, 300, 60.0, noise=2.0)
    cells = _cells(g, 16.0)
    assert cells[0] == 16.0
    want = _against_the_rule(g, nrm, Y, 16.0, 6, cells=cells)
    assert want[2].max() > 20 and want[1].any()


def test_two_runs_give_the_same_bytes():
    g, nrm, Y = _sheet(12, 3000, 30.0)
    cells = _cells(g, 3.0)
    order = register.cell_order(torch.from_numpy(g), cells).numpy()
    a, b = (Call(g[order], nrm[order], Y[order], cells, 3.0, 6).arrays() for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1].any()


def test_bad_input_raises_the_flag_and_the_next_call_clears_it():
    g, nrm, Y = _sheet(13, 400, 10.0)
    cells = _cells(g, 2.0)
    order = register.cell_order(torch.from_numpy(g), cells).numpy()
    g, nrm, Y = g[order], nrm[order], Y[order]
    ws = Call(g, nrm, Y, cells, 2.0, 4).ws
    want = ref.gradient(g, nrm, Y, 2.0, 4)
    nan = g.copy()
    nan[123, 1] = np.nan
    outside = g.copy()
    outside[7] = g.max(0) + 100.0
    loud = Y.copy()
    loud[200] = ref.Y_MAX + 1
    for bad_g, bad_Y in ((g[::-1].copy(), Y), (nan, Y), (outside, Y), (g, loud), (g, -Y - 1)):
        call = Call(bad_g, nrm, bad_Y, cells, 2.0, 4, ws=ws)
        assert call.rc == 0 and (call.arrays()[1] == register.GRADIENT_BAD_INPUT).all()
        with pytest.raises(RuntimeError, match="pcgc_color_gradient: a coordinate is not finite or leaves the cells"):
            register.color_gradient_step(torch.from_numpy(bad_g).cuda(), torch.from_numpy(nrm).cuda(), torch.from_numpy(bad_Y).cuda(), cells,
                                         2.0, 4)
        again = Call(g, nrm, Y, cells, 2.0, 4, ws=ws)
        grad, valid, K, Q, B = again.arrays()
        assert again.rc == 0 and grad.tobytes() == want[0].tobytes() and np.array_equal(valid, want[1]) and np.array_equal(B, want[4])


def test_every_bad_argument_of_the_gradient_is_refused():
    lib = _lib.hip()
    dev = torch.device("cuda")
    n = 10
    g = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    nrm, Y = torch.ones_like(g), torch.zeros(n, dtype=torch.int32, device=dev)
    grad, valid = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    K, Q, B = (torch.zeros(n * w, dtype=t, device=dev) for w, t in ((1, torch.int32), (6, torch.int64), (3, torch.int64)))
    ws = torch.empty(int(lib.pcgc_color_gradient_workspace_bytes(4, n)), dtype=torch.uint8, device=dev)
    good = dict(points=g, normals=nrm, Y=Y, n=n, h=2.0, ox=0, oy=0, oz=0, res=4, radius=1.5, kmin=6, g=grad, valid=valid, K=K, Q=Q, B=B,
                ws=ws, ws_bytes=ws.numel())

    def call(**change):
        a = dict(good, **change)
        return lib.pcgc_color_gradient(_lib.dptr(a["points"]), _lib.dptr(a["normals"]), _lib.dptr(a["Y"]), a["n"], a["h"], a["ox"], a["oy"],
                                       a["oz"], a["res"], a["radius"], a["kmin"], _lib.dptr(a["g"]), _lib.dptr(a["valid"]), _lib.dptr(a["K"]),
                                       _lib.dptr(a["Q"]), _lib.dptr(a["B"]), _lib.dptr(a["ws"]), a["ws_bytes"], _lib.stream())

    assert call() == 0 and call(K=None, Q=None, B=None) == 0
    torch.cuda.synchronize()
    for change in (dict(points=None), dict(normals=None), dict(Y=None), dict(g=None), dict(valid=None), dict(ws=None), dict(n=0), dict(n=-1),
                   dict(n=2 ** 31), dict(res=0), dict(res=1025), dict(h=3.0), dict(h=0.5), dict(h=float("nan")), dict(ox=2 ** 29),
                   dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=2.5),
                   dict(radius=16.5, h=32.0), dict(kmin=2), dict(kmin=(1 << 20) + 1), dict(K=None), dict(Q=None), dict(B=None),
                   dict(K=None, Q=None), dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0)):
        assert call(**change) != 0, change
        assert lib.pcgc_last_error().decode().startswith("pcgc_color_gradient: "), change
    assert call(radius=16.0, h=16.0) == 0 and call(kmin=1 << 20) == 0
    torch.cuda.synchronize()
    for res, m in ((0, 10), (1025, 10), (4, 0), (4, -3), (4, 2 ** 31)):
        assert lib.pcgc_color_gradient_workspace_bytes(res, m) == 0
    assert lib.pcgc_color_gradient_workspace_bytes(4, 10) == lib.pcgc_smooth_workspace_bytes(4, 10) > 0


# ---------------------------------------------------------------------------- kernel 2: one step
def _pose_about(c, small=True):
    """a rotation about the centre c and a shift, with entries that are not float32 numbers"""
    R = rr.rodrigues(np.array([0.01, -0.02, 0.015]) if small else np.array([0.3, -0.2, 0.25]))
    return R, c - R @ c + np.array([0.3, -0.2, 0.1])


def _check_step(source, cs, target, normals, ct, R, t, max_dist, what, kmin=6, radius=3.0):
    """a step on the device against the reference by brute force: n_used, best, ties and the count of valid pairs equal, every
    sum within the summation bound; the gradients the matcher fitted are the rule's"""
    m = register.ColorMatcher(source, target, normals, cs, ct, radius, kmin)
    c = m.centre
    if R is None:
        R, t = _pose_about(c)
    S, best, ties = m.step(R, t, c, max_dist, per_point=True)
    unit = register._unit_normals(normals, len(target))
    Yp, Yq = ref.intensity(cs), ref.intensity(ct)
    grad, valid = ref.gradient(target, unit, Yq, radius, kmin)[:2]
    order = m.cells.order.cpu().numpy()
    assert m.grad_d.cpu().numpy().tobytes() == grad[order].tobytes() and np.array_equal(m.valid_d.cpu().numpy(), valid[order])
    want = ref.step(source, Yp, target, unit, Yq, grad, valid, R, t, c, max_dist)
    assert len(S) == 59 and S[0] == want["S"][0], (what, S[0], want["S"][0])
    assert best.tobytes() == want["best"].tobytes(), (what, int((best != want["best"]).sum()))
    assert np.array_equal(ties, want["ties"]), what
    err, bound = np.abs(S - want["S"]), ref.bound(want)
    print(what, "n_used %d, valid weight %.6g, largest error / bound %.3g" % (S[0], S[30], float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), (what, np.nonzero(err > bound)[0].tolist())
    if np.isin(want["ties"], (0, 1, 2, 4, 8)).all():
        assert S[30] == want["S"][30]                          # every weight a power of two: any order of additions is exact
    return S, want, m


def _bumpy():
    d = ref.fixture("bumpy")
    return d["source"], d["source_colors"], d["target"], d["target_normals"], d["target_colors"]


@pytest.mark.parametrize("posed", (False, True))
@pytest.mark.parametrize("n", (1, 63, 257))
def test_step_sizes(n, posed):
    """less than a wave, more than a workgroup; at identity, and under a pose whose result is rounded to float32.  The source
    rows are those nearest to the target, so that the cloud of one point is inside the gate"""
    s, cs, t, nrm, ct = _bumpy()
    if "near" not in _CACHE:
        _CACHE["near"] = np.argsort(rr.step(s, t, None, np.eye(3), np.zeros(3), np.zeros(3), 100.0)["best"], kind="stable")
    rows = _CACHE["near"][:n]
    pose = (None, None) if posed else (np.eye(3), np.zeros(3))
    S, want, _ = _check_step(s[rows], cs[rows], t, nrm, ct, *pose, 2.0, "n = %d, posed %s" % (n, posed))
    assert S[0] >= 1 and S[30] > 0 and S[58] > 0 and S[31:52].any()


def _lattice_case():
    """4 000 source points half a voxel off the integer lattice the target lies on: two and more tied neighbours"""
    if "lattice" not in _CACHE:
        d = ref.fixture("sphere")
        q = np.unique(np.rint(d["target"].astype(np.float64)), axis=0)
        nrm = q - 32.0
        p = np.concatenate([q + np.array([0.5, 0.0, 0.0]), q + np.array([0.0, 0.5, 0.0])])[:4000]
        _CACHE["lattice"] = (p.astype(np.float32), ref.texture(p), q.astype(np.float32), nrm.astype(np.float32), ref.texture(q))
    return _CACHE["lattice"]


def test_four_thousand_points_with_ties():
    p, cp, q, nrm, cq = _lattice_case()
    S, want, _ = _check_step(p, cp, q, nrm, cq, np.eye(3), np.zeros(3), 1.5, "lattice")
    assert len(p) == 4000 and want["ties"].max() == 2 and (want["ties"] == 2).sum() > 100 and S[30] > 100


def test_gate_equal_to_a_distance_and_a_source_outside_the_box():
    """best = 9 exactly: max_dist = 3 uses the point, the next number below 3 does not; the point lies outside the target's box"""
    g, nrm, _ = _sheet(21, 300, 8.0)
    g = np.concatenate([g, np.array([[4, 4, 12]], np.float32)])           # a point alone above the sheet, and the source above it
    nrm = np.concatenate([nrm, np.array([[0, 0, 1]], np.float32)])
    ct = ref.texture(g)
    p = np.array([[4, 4, 15]], np.float32)
    assert g[:-1, 2].max() < 9.0
    cp = np.array([[10, 200, 30]], np.uint8)
    eye = (np.eye(3), np.zeros(3))
    S, want, _ = _check_step(p, cp, g, nrm, ct, *eye, 3.0, "gate = distance", kmin=4)
    assert S[0] == 1 and S[1] == 9.0 and want["ties"].tolist() == [1]
    S, want, _ = _check_step(p, cp, g, nrm, ct, *eye, float(np.nextafter(3.0, 0.0)), "gate below distance", kmin=4)
    assert want["best"].tolist() == [9.0] and want["ties"].tolist() == [0] and not S.any()


def test_some_and_all_gradients_invalid():
    s, cs, t, nrm, ct = _bumpy()
    S, want, m = _check_step(s[:257], cs[:257], t, nrm, ct, None, None, 2.0, "kmin 70", kmin=70)
    assert 0 < m.n_valid < m.m and 0 < S[30] < S[0]
    S, want, m = _check_step(s[:257], cs[:257], t, nrm, ct, None, None, 2.0, "kmin 2^20", kmin=1 << 20)
    assert m.n_valid == 0 and S[0] > 10 and S[2:30].all() and not S[30:].any() and not want["S"][30:].any()


def test_the_search_is_that_of_the_plain_step():
    """S[0], the sum of best and the per-point outputs equal pcgc_register_step's on the same inputs"""
    s, cs, t, nrm, ct = _bumpy()
    cm = register.ColorMatcher(s, t, nrm, cs, ct)
    pm = register.Matcher(s, t, nrm)
    R, tt = _pose_about(cm.centre, small=False)
    Sc, bc, tc = cm.step(R, tt, cm.centre, 1.5, per_point=True)
    Sp, bp, tp = pm.step(R, tt, pm.centre, 1.5, per_point=True)
    assert Sc[0] == Sp[0] > 100 and Sc[1] == Sp[1] and bc.tobytes() == bp.tobytes() and np.array_equal(tc, tp)
    assert Sc[2:30].tobytes() == Sp[17:45].tobytes()          # the same terms in the same order
    cm.sort_source(R, tt)                                      # the intensities travel with the sorted source
    S2, b2, t2 = cm.step(R, tt, cm.centre, 1.5, per_point=True)
    assert b2.tobytes() == bc.tobytes() and np.array_equal(t2, tc) and S2[0] == Sc[0] and S2[30] == Sc[30]
    assert np.allclose(S2, Sc, rtol=1e-9, atol=1e-12) and not np.array_equal(cm.source_d.cpu().numpy(), s)


def test_two_runs_give_the_same_bits():
    p, cp, q, nrm, cq = _lattice_case()
    m = register.ColorMatcher(p, q, nrm, cp, cq)
    R, t = _pose_about(m.centre)
    first = m.step(R, t, m.centre, 1.5)
    assert first.tobytes() == m.step(R, t, m.centre, 1.5).tobytes()
    assert first.tobytes() == register.ColorMatcher(p, q, nrm, cp, cq).step(R, t, m.centre, 1.5).tobytes()


def test_nan_source_fails_that_step_only():
    s, cs, t, nrm, ct = _bumpy()
    bad = s[:257].copy()
    bad[100, 1] = np.nan
    m = register.ColorMatcher(bad, t, nrm, cs[:257], ct)
    with pytest.raises(RuntimeError, match="pcgc_register_color_step"):
        m.step(np.eye(3), np.zeros(3), m.centre, 1.5)
    good = register.ColorMatcher(s[:257], t, nrm, cs[:257], ct)
    first = good.step(np.eye(3), np.zeros(3), good.centre, 1.5)
    with pytest.raises(RuntimeError, match="pcgc_register_color_step"):
        good.step(np.eye(3), np.full(3, np.float64(3e38)), good.centre, 1.5)
    assert np.array_equal(good.step(np.eye(3), np.zeros(3), good.centre, 1.5), first)      # the flag is the step's own


def test_bad_arguments_of_the_step_are_refused():
    s, cs, t, nrm, ct = _bumpy()
    m = register.ColorMatcher(s[:63], t, nrm, cs[:63], ct)
    for R, tt, c, gate in ((np.eye(3), np.zeros(3), m.centre, 0.0), (np.eye(3), np.zeros(3), m.centre, float("inf")),
                           (np.eye(3), np.zeros(3), m.centre, float("nan")), (np.eye(3) * np.nan, np.zeros(3), m.centre, 1.0),
                           (np.eye(3), np.array([0, np.inf, 0]), m.centre, 1.0), (np.eye(3), np.zeros(3), np.array([np.nan, 0, 0]), 1.0)):
        with pytest.raises(_lib.PcgcError, match="pcgc_register_color_step"):
            m.step(R, tt, c, gate)
    lib = _lib.hip()
    assert lib.pcgc_register_color_workspace_bytes(0, 10) == 0 and lib.pcgc_register_color_workspace_bytes(8, 0) == 0
    assert lib.pcgc_register_color_workspace_bytes(8, 10) == lib.pcgc_offgrid_workspace_bytes(8, 10) + 59 * 1024 * 8
    R9, z3 = np.eye(3).reshape(9).copy(), np.zeros(3)
    good = [m.source_d, m.Yp_d, m.cells.points, m.normals_d, m.Yq_d, m.grad_d, m.valid_d]

    def call(tensors, ws_bytes):
        a = [_lib.dptr(x) for x in tensors]
        return lib.pcgc_register_color_step(a[0], a[1], m.n, a[2], a[3], a[4], a[5], a[6], m.m, *m.cells.grid(), _lib.nptr(R9), _lib.nptr(z3),
                                            _lib.nptr(z3), 1.0, _lib.dptr(m.out), None, None, _lib.dptr(m.ws), ws_bytes, _lib.stream())

    assert call(good, m.ws.numel()) == 0
    torch.cuda.synchronize()
    for k in range(len(good)):                                 # every array is required, the target's normals among them
        assert call(good[:k] + [None] + good[k + 1:], m.ws.numel()) != 0
        assert lib.pcgc_last_error().decode().startswith("pcgc_register_color_step: ")
    assert call(good, m.ws.numel() - 1) != 0 and "workspace too small" in lib.pcgc_last_error().decode()


# ---------------------------------------------------------------------------- the loop
def _apart(a, b, points):
    p = np.asarray(points, np.float64)
    return float(np.linalg.norm((p @ a["R"].T + a["t"]) - (p @ b["R"].T + b["t"]), axis=1).max())


# the largest distance between a source point under the device's pose and under the reference's, measured on the three
# fixtures on the MI355X (DESIGN.md §7k, next to §7h's 3.9e-8).  The test allows ten times the largest of them.
MEASURED_APART = {"flat": 3.18e-14, "sphere": 7.11e-15, "bumpy": 8.7e-15}
RECORDED = {"flat": 0.00433, "sphere": 0.00456, "bumpy": 0.01866}       # the reference's truth errors


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_loop_follows_the_reference(name):
    d = ref.fixture(name)
    want = ref.reference_loop(name)
    got = register.icp(d["source"], d["target"], d["target_normals"], "color", source_colors=d["source_colors"],
                       target_colors=d["target_colors"])
    apart, err = _apart(got, want, d["source"]), ref.truth_error(got, d)
    print("%s: steps %s, n_used %d, device and reference %.3g voxel apart, truth error %.5f voxel, colour rmse %.5f, fitness %.4f" % (
        name, got["iterations"], got["n_used"], apart, err, got["color_rmse"], got["color_fitness"]))
    assert got["iterations"] == want["iterations"] and got["converged"] and want["converged"]
    assert got["n_used"] == want["n_used"] and got["fitness"] == want["fitness"]
    assert apart <= 10.0 * max(MEASURED_APART.values())
    assert err <= 2.0 * RECORDED[name]
    assert abs(got["rmse"] - want["rmse"]) < 1e-6 and abs(got["plane_rmse"] - want["plane_rmse"]) < 1e-6
    assert abs(got["color_rmse"] - want["color_rmse"]) < 1e-6 and abs(got["color_fitness"] - want["color_fitness"]) < 1e-9


def test_geometry_alone_on_the_device_fails_where_the_reference_says():
    d = ref.fixture("flat")
    with pytest.raises(ValueError, match="use metric='color' when the scans carry texture"):
        register.icp(d["source"], d["target"], d["target_normals"], "plane")
    d = ref.fixture("sphere")
    r = register.icp(d["source"], d["target"], d["target_normals"], "plane", iters=10)
    assert ref.truth_error(r, d) >= 1.0


# ---------------------------------------------------------------------------- through the layers
UNIT = 0.01                  # scanner units per unit of the surface generator
VOXEL = 0.01                 # the voxel edge the three scans are merged at


def _write_scan(name, points, colors, normals):
    """an ASCII ply with colours and normals; repr keeps every float64 and float32 as it is"""
    with open(name, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\nproperty uchar red\n"
                "property uchar green\nproperty uchar blue\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(points))
        for p, c, n in zip(points.tolist(), colors.tolist(), normals.astype(np.float64).tolist()):
            f.write("%r %r %r %d %d %d %r %r %r\n" % (p[0], p[1], p[2], c[0], c[1], c[2], n[0], n[1], n[2]))


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """the three textured scans as plies, read back, and register_scans(metric="color") on them; once"""
    from pcgcv1_amd.dataprocess.inout_points import load_ply_scan
    folder = tmp_path_factory.mktemp("color_scans")
    scans, _ = ref.three_textured_scans(unit=UNIT)
    names = [str(folder / ("scan%d.ply" % k)) for k in range(3)]
    loaded = []
    for name, (p, col, nrm) in zip(names, scans):
        _write_scan(name, p, col, nrm)
        back = load_ply_scan(name)
        assert np.array_equal(back[0], p) and np.array_equal(back[1], col) and back[2].tobytes() == nrm.tobytes()
        loaded.append(back)
    return names, loaded, register.register_scans(loaded, voxel_size=VOXEL, metric="color")


def test_register_scans_equals_chained_icp_calls(three):
    _, scans, out = three
    pts, cols, nrms = [scans[0][0]], [scans[0][1]], [scans[0][2]]
    assert "color_rmse" not in out["poses"][0]
    for k, (p, col, nrm) in enumerate(scans[1:], 1):
        target = np.concatenate(pts)
        frame = ingest.fit_frame(target, voxel_size=VOXEL)
        r = register.icp(register.to_grid(p, frame), register.to_grid(target, frame), np.concatenate(nrms), "color", source_colors=col,
                         target_colors=np.concatenate(cols))
        R, t = register.pose_to_scan_units(r["R"], r["t"], frame)
        got = out["poses"][k]
        print("scan %d: steps %s, fitness %.3f, colour rmse %.4f, colour fitness %.3f" % (k, got["iterations"], got["fitness"],
                                                                                        got["color_rmse"], got["color_fitness"]))
        assert got["converged"] and got["R"].tobytes() == R.tobytes() and got["t"].tobytes() == t.tobytes()
        assert got["iterations"] == r["iterations"] and got["n_used"] == r["n_used"]
        assert got["color_rmse"] == r["color_rmse"] and got["color_fitness"] == r["color_fitness"] and 0 < got["color_fitness"] <= 1
        pts.append(p @ R.T + t)
        cols.append(col)
        nrms.append((nrm.astype(np.float64) @ R.T).astype(np.float32))
    assert np.array_equal(out["aligned"][0], np.concatenate(pts)) and np.array_equal(out["aligned"][1], np.concatenate(cols))
    # the poses are the ones that moved the scans, undone: every point within a twentieth of a voxel of where it was sampled
    _, poses = ref.three_textured_scans(unit=UNIT)
    for k in (1, 2):
        true = (scans[k][0] / UNIT - poses[k][1]) @ poses[k][0]
        assert np.abs(scans[k][0] @ out["poses"][k]["R"].T + out["poses"][k]["t"] - true * UNIT).max() / VOXEL < 0.1


def test_command_line_writes_the_same_poses_and_the_new_figures(three, tmp_path, capsys):
    from pcgcv1_amd.dataprocess.inout_points import write_ply_data
    names, scans, out = three
    merged = str(tmp_path / "merged.ply")
    register.main(["--input"] + names + ["--output", merged, "--voxel_size", repr(VOXEL), "--metric", "color"])
    printed = capsys.readouterr().out
    assert printed.count(", colour rmse ") == 2 and printed.count(", colour fitness ") == 2 and "wrote " in printed
    poses = register.read_poses(register.poses_path(merged))
    for k, (e, r) in enumerate(zip(poses, out["poses"])):
        assert e["pose"].tobytes() == r["pose"].tobytes() and e["iterations"] == r["iterations"]
        assert ("color_rmse" in e) == ("color_fitness" in e) == (k > 0)
        if k:
            assert e["color_rmse"] == r["color_rmse"] and e["color_fitness"] == r["color_fitness"] and e["plane_rmse"] == r["plane_rmse"]
    # the options reach the loop: another weight, other figures
    other = str(tmp_path / "other.ply")
    register.main(["--input"] + names[:2] + ["--output", other, "--voxel_size", repr(VOXEL), "--metric", "color", "--color_weight", "0.5",
                   "--color_radius", "2", "--color_kmin", "4"])
    assert ", colour rmse " in capsys.readouterr().out
    assert register.read_poses(register.poses_path(other))[1]["pose"].tobytes() != poses[1]["pose"].tobytes()
    # the plane metric's entries stay as they were
    plain = str(tmp_path / "plain.ply")
    register.main(["--input"] + names[:2] + ["--output", plain, "--voxel_size", repr(VOXEL)])
    assert "colour" not in capsys.readouterr().out
    assert all("color_rmse" not in e and "color_fitness" not in e for e in register.read_poses(register.poses_path(plain)))
    # scans without colours are an argument error before a file is parsed
    bare = str(tmp_path / "bare.ply")
    write_ply_data(bare, np.rint(scans[1][0] / UNIT).astype(np.int32))
    with open(bare, "ab") as f:
        f.write(b"not a vertex\n")
    with pytest.raises(SystemExit):
        register.main(["--input", names[0], bare, "--output", str(tmp_path / "bad.ply"), "--voxel_size", repr(VOXEL), "--metric", "color"])
    assert "--metric=color needs colours: %s" % bare in capsys.readouterr().err and not os.path.exists(str(tmp_path / "bad.ply"))
