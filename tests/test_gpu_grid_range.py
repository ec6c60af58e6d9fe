"""The oldest kernels of the shared voxel grid at the top of their range: pcgc_d1_mse, pcgc_d2_transfer_normals and pcgc_d2_mse
(csrc/tail.hip), pcgc_recolor and pcgc_color_mse (csrc/color.hip) and pcgc_estimate_normals (csrc/mesh.hip) on grids whose cell
index does not fit 31 or 32 bits, and their grid-stride loops on a second sweep.  (pcgc_mesh_voxelize at resolutions 2047 and
4095 is a line of tests/test_gpu_mesh2pc.py, against the reference it already has.)

One table, TABLE: entry point x grid.  Grids: res 1291 and 1626, the first whose last cell has a key >= 2^31 and >= 2^32 (no
powers of two: the key decode divides), 2048, and 4096, the top of the range (2^36 cells, a bit set of 8 GiB; 16 GiB with the rank
table of the colour kernels).  Every case of the table runs
  * the faces pair of tests/_clouds.py at that res against brute force in numpy;
  * the frozen cases of tests/test_gpu_d1d2_exact.py moved by res - r0 into the far corner: every operation depends on differences
    of coordinates and the order of the points only, so every output equals the unmoved run's bit for bit, FROZEN_D2 and
    FROZEN_COLOR_MSE_FACES_RES64 included;
  * both ends at once: the unmoved and the moved copy as one cloud, so keys and ranks span the whole set;
  * at res 2048 and 4096 the alias decoys.  An index cut to 31 or 32 bits in the writer and the reader alike agrees with itself
    and passes all of the above unless two cells collide, so queries stand where a cut index would put a ghost of the far block:
    2^31 / res^2 and 2^32 / res^2 cells before it in x, their true nearest target 4 to 6 cells away and nothing nearer.
The second-sweep cases take a checkerboard of side 130 (1 098 500 cells per parity: more than 4096 workgroups of 256 points, the
largest launch of recolor_scatter_kernel and d2_transfer_kernel, and four sweeps of the 1024-workgroup reductions) against the
stencil reference tests/_grid_ref.py.

nearest_d2 walks Chebyshev shells at cubic cost: a query 2000 cells from its target runs for minutes and would be taken for a
hang.  So every input here is built, and every query's nearest target shown to be at most 8 cells away, BEFORE anything is
launched (_near; the stencil reference asserts d^2 <= 9 itself).  Keep it so in every case added here.
"""
import contextlib
import functools
import gc
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as cref                                                # noqa: E402
import _grid_ref as gref                                                 # noqa: E402
from _clouds import faces                                                # noqa: E402
from test_gpu_d1d2_exact import (D2_CASES, FROZEN_COLOR_MSE_FACES_RES64, FROZEN_D2, _d2_device, _dist2,    # noqa: E402
                                 _plane)
from test_gpu_mesh2pc import _check_normals                              # noqa: E402
from pcgcv1_amd import _lib, metrics                                     # noqa: E402
from pcgcv1_amd import recolor as rc                                     # noqa: E402

GRIDS = (1291, 1626, 2048, 4096)
ENTRIES = ("d1", "d2", "recolor", "color_mse", "normals")
TABLE = [pytest.param(entry, res, id="%s-res%d" % (entry, res)) for res in GRIDS for entry in ENTRIES]
DECOY_SHIFTS = {2048: (512, 1024), 4096: (128, 256)}        # 2^31 / res^2 and 2^32 / res^2 cells in x
MAX_NEAR_D2 = 64                                            # no query farther than 8 cells from its nearest target
SWEEP_RES, SWEEP_SIDE = 2048, 130
BIT_SETS = {"d1": 1, "d2": 1, "recolor": 2, "color_mse": 2, "normals": 1}      # res^3 / 8 bytes each (bits; bits and rank)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(autouse=True)
def _one_case_at_a_time(request):
    """The top-of-range cases hold 8 or 16 GiB: they run one after the other on a freed device.  Prints what
    profiles/grid_range_tests.txt records (run with -s): seconds and peak device bytes of the case."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\nGRID_RANGE %-60s %7.2f s  peak %8.1f MiB" % (request.node.name, time.perf_counter() - t0,
                                                          torch.cuda.max_memory_allocated() / 2.0 ** 20))
    gc.collect()
    torch.cuda.empty_cache()


def _workspace_bytes(entry, res, n):
    lib = _lib.hip()
    return int({"d1": lambda: lib.pcgc_d1_workspace_bytes(res), "d2": lambda: lib.pcgc_d2_workspace_bytes(res, n),
                "recolor": lambda: lib.pcgc_recolor_workspace_bytes(res, n, n), "color_mse": lambda: lib.pcgc_color_mse_workspace_bytes(res, n),
                "normals": lambda: lib.pcgc_normals_workspace_bytes(res, n, 10.0)}[entry]())


@contextlib.contextmanager
def _device_memory(entry, res, n):
    """a refused allocation is a failure that names the sizes, not a skip"""
    try:
        yield
    except torch.cuda.OutOfMemoryError as e:
        free, total = torch.cuda.mem_get_info()
        pytest.fail("%s at res %d: the device refused an allocation: the workspace is %d bytes (%d bit sets of %d bytes), %d of %d "
                    "bytes are free: %s" % (entry, res, _workspace_bytes(entry, res, n), BIT_SETS[entry], res ** 3 // 8, free, total, e))


# ---------------------------------------------------------------------------------------------------------------- inputs
def _key_order(p):
    return np.lexsort((p[:, 2], p[:, 1], p[:, 0]))


def _keys(p, res):
    p = np.asarray(p, np.int64)
    return (p[:, 0] * res + p[:, 1]) * res + p[:, 2]


def _near(a, b):
    """the largest squared distance from a point of a to its nearest point of b (brute force, 512 queries at a time); the
    assertion that keeps the shell search short"""
    worst = max(int(_dist2(a[i:i + 512], b).min(1).max()) for i in range(0, len(a), 512))
    assert worst <= MAX_NEAR_D2, "a query lies %d (squared) from its nearest target: the shell search would run for minutes" % worst
    return worst


class Pair(object):
    """cloud A (points, colours, normals) and cloud B (points, colours); near = the largest nearest d^2 either way"""

    def __init__(self, a, ca, na, b, cb, near=None):
        self.a, self.ca, self.na, self.b, self.cb = (np.ascontiguousarray(x) for x in (a, ca, na, b, cb))
        assert self.a.dtype == np.int32 and self.b.dtype == np.int32 and len(a) == len(ca) == len(na) and len(b) == len(cb)
        self.near = max(_near(self.a, self.b), _near(self.b, self.a)) if near is None else near

    def moved(self, offset):
        """distances are differences of coordinates: the bound moves along"""
        return Pair(self.a + np.int32(offset), self.ca, self.na, self.b + np.int32(offset), self.cb, near=self.near)

    def with_copy_at(self, offset, side):
        """this pair and its copy moved by `offset` as one cloud each; the copies are farther apart than any nearest distance"""
        assert offset - side > 2 * 8 and self.a.max() < side and self.b.max() < side
        far = self.moved(offset)
        return Pair(np.r_[self.a, far.a], np.r_[self.ca, self.ca], np.r_[self.na, self.na], np.r_[self.b, far.b], np.r_[self.cb, self.cb],
                    near=self.near)


def _normals_for(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)


def _colors_for(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _frozen_pairs():
    """name -> (Pair, r0): the D2 cases with their own normals (FROZEN_D2 is theirs) and seeded colours, the faces_res64 colour
    pair with its own colours (FROZEN_COLOR_MSE_FACES_RES64 is theirs) and seeded normals"""
    out = {}
    for i, name in enumerate(sorted(D2_CASES)):
        a, na, b, r0 = D2_CASES[name]
        out[name] = (Pair(a, _colors_for(200 + i, len(a)), na, b, _colors_for(300 + i, len(b))), r0)
    (a, ca), (b, cb) = faces(10, 64, 1500), faces(11, 64, 1200)
    out["faces_res64"] = (Pair(a, ca, _normals_for(110, len(a)), b, cb), 64)
    return out


@functools.lru_cache(maxsize=None)
def _faces_pair(res):
    (a, ca), (b, cb) = faces(10, res, 1500), faces(11, res, 1200)
    return Pair(a, ca, _normals_for(res, len(a)), b, cb)


@functools.lru_cache(maxsize=None)
def _decoy_pair(res):
    """The far block (dense_res12 in the far corner) and, per shift, queries at the positions of its targets' first three
    x-planes minus the shift: a cut index puts a ghost of the block's targets exactly there.  Their true nearest target is a
    plane of anchors 4 cells before the block's place, straight across: 4, 5 or 6 cells, and nothing nearer."""
    base, r0 = _frozen_pairs()["dense_res12"]
    far = base.moved(res - r0)
    qs, planes = [], []
    g = np.arange(res - r0, res)
    for shift in DECOY_SHIFTS[res]:
        front = far.b[far.b[:, 0] < res - r0 + 3]
        qs.append(front - np.int32([shift, 0, 0]))
        yy, zz = np.meshgrid(g, g, indexing="ij")
        planes.append(np.stack([np.full(yy.size, res - r0 - shift - 4), yy.ravel(), zz.ravel()], -1).astype(np.int32))
    q, pl = np.concatenate(qs), np.concatenate(planes)
    assert len(q) > 100
    # the decoys' own nearest targets: 4 to 6 cells, alone at that distance
    d = _dist2(q, np.r_[far.b, pl])
    assert set(np.unique(d.min(1)).tolist()) == {16, 25, 36} and ((d == d.min(1, keepdims=True)).sum(1) == 1).all()
    a, b = np.r_[far.a, q], np.r_[far.b, pl]
    return Pair(a, np.r_[far.ca, _colors_for(400, len(q))], np.r_[far.na, _normals_for(401, len(q))], b, np.r_[far.cb, _colors_for(402, len(pl))])


# ---------------------------------------------------------------------------------------------------------------- device
def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_lib.require_gpu())


def _run_d1(p, res):
    a_d, b_d = _dev(p.a), _dev(p.b)
    ws = torch.empty(int(_lib.hip().pcgc_d1_workspace_bytes(res)), dtype=torch.uint8, device=a_d.device)
    return {"d1": np.array(metrics._d1_one_way(a_d, b_d, res, ws) + metrics._d1_one_way(b_d, a_d, res, ws))}


def _run_d2(p, res):
    """both D2 calls as metrics.d2_metrics makes them, on the clouds in key order; B's normals back in B's own order"""
    oa, ob = _key_order(p.a), _key_order(p.b)
    nb_sorted, out = _d2_device(p.a[oa], p.na[oa], p.b[ob], res)
    nb = np.empty_like(nb_sorted)
    nb[ob] = nb_sorted
    return {"normals_b": nb, "d2": out}


def _run_recolor(p, res):
    colors, counts = rc.recolor(p.a, p.ca, p.b, res, return_counts=True)
    return {"colors": colors, "counts": counts}


def _run_color_mse(p, res):
    lib, st = _lib.hip(), _lib.stream()
    (pa, ca), (pb, cb) = ((_dev(x), _dev(c)) for x, c in ((p.a, p.ca), (p.b, p.cb)))
    out = torch.empty(6, dtype=torch.float64, device=pa.device)
    ws = torch.empty(int(lib.pcgc_color_mse_workspace_bytes(res, max(len(p.a), len(p.b)))), dtype=torch.uint8, device=pa.device)
    _lib.check(lib.pcgc_color_mse(_lib.dptr(pa), _lib.dptr(ca), len(p.a), _lib.dptr(pb), _lib.dptr(cb), len(p.b), res, _lib.dptr(out),
                                  _lib.dptr(ws), ws.numel(), st), "pcgc_color_mse A->B")
    _lib.check(lib.pcgc_color_mse(_lib.dptr(pb), _lib.dptr(cb), len(p.b), _lib.dptr(pa), _lib.dptr(ca), len(p.a), res, _lib.dptr(out[3:]),
                                  _lib.dptr(ws), ws.numel(), st), "pcgc_color_mse B->A")
    return {"color_mse": out.cpu().numpy()}


RUN = {"d1": _run_d1, "d2": _run_d2, "recolor": _run_recolor, "color_mse": _run_color_mse}
EXACT = ("d1", "normals_b", "colors", "counts")             # integer rules: equal; the rest are float64 sums: 1e-12 relative


def _run(entry, p, res):
    assert p.near <= MAX_NEAR_D2 and min(p.a.min(), p.b.min()) >= 0 and max(p.a.max(), p.b.max()) < res       # before any launch
    with _device_memory(entry, res, max(len(p.a), len(p.b))):
        return RUN[entry](p, res)


def _same_bytes(got, want, what):
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


def _agree(got, want, what):
    """got against a reference that holds at least got's keys: integers equal, float64 sums within 1e-12 relative"""
    for k, g in got.items():
        w = want[k]
        print(what, k, g if g.size <= 6 else g.shape, w if w.size <= 6 else "")
        if k in EXACT:
            assert g.shape == w.shape and np.array_equal(g, w), (what, k, int((g != w).sum()))
        else:
            assert np.all(np.abs(g - w) <= 1e-12 * np.abs(w)), (what, k, g, w)


# ---------------------------------------------------------------------------------------------------------------- references
def _brute_force(p):
    """every output of the four entry points for a pair of a few thousand points, as the existing exact tests state them"""
    d = _dist2(p.a, p.b)
    tie_ab, tie_ba = d == d.min(1, keepdims=True), (d == d.min(0, keepdims=True)).T
    d1 = []
    for near in (d.min(1), d.min(0)):
        d1 += [float(np.float64(int(near.sum())) / np.float64(len(near))), float(near.max())]
    fixed = np.rint(p.na.astype(np.float64) * 2.0 ** 40).astype(np.int64)
    sums, count = tie_ab.T.astype(np.int64) @ fixed, tie_ab.sum(0)
    nb = np.where(count[:, None] > 0, sums.astype(np.float64) / 2.0 ** 40 / np.maximum(count, 1)[:, None], 0.0).astype(np.float32)
    p_ab, p_ba = _plane(p.a, p.b, nb, tie_ab), _plane(p.b, p.a, p.na, tie_ba)
    colors, counts = cref.recolor(p.a, p.ca, p.b)
    return {"d1": np.array(d1), "normals_b": nb, "d2": np.array([p_ab.mean(), p_ab.max(), p_ba.mean(), p_ba.max()]),
            "colors": colors, "counts": counts,
            "color_mse": np.r_[cref.color_mse(p.a, p.ca, p.b, p.cb), cref.color_mse(p.b, p.cb, p.a, p.ca)]}


@functools.lru_cache(maxsize=None)
def _faces_reference(res):
    return _brute_force(_faces_pair(res))


@functools.lru_cache(maxsize=None)
def _decoy_reference(res):
    return _brute_force(_decoy_pair(res))


def _twice(single):
    """what the two copies of a pair give as one cloud, from what one copy gives: per-point outputs concatenated, D1 the
    weighted mean of two equal integer sums (the same double), the maxima the same, the float64 means to rounding"""
    return {k: np.r_[v, v] if k in ("normals_b", "colors", "counts") else v for k, v in single.items()}


# ---------------------------------------------------------------------------------------------------------------- the table
def _normals_case(res):
    """clusters at both ends of the key range, one through the cell (res-1, res-1, res-1), and where a cut index would put the far
    cluster's ghost a cluster of another shape; covariances and neighbour counts exact against tests/_mesh_ref.py"""
    base, r0 = _frozen_pairs()["dense_res12"]
    far = base.a + np.int32(res - r0)
    parts = [far, np.int32([[res - 1, res - 1, res - 1], [res - 2, res - 1, res - 1]]), base.b]
    for shift in DECOY_SHIFTS.get(res, ()):
        parts.append(base.b + np.int32(res - r0) - np.int32([shift, 0, 0]))
    pts = np.unique(np.concatenate(parts), axis=0).astype(np.int32)
    pts = pts[np.random.default_rng(res).permutation(len(pts))]
    assert pts.max() == res - 1 and (_keys(pts, res) >= 2 ** 31).any() and (res < 1626 or (_keys(pts, res) >= 2 ** 32).any())
    with _device_memory("normals", res, len(pts)):
        _check_normals(pts)


@pytest.mark.parametrize("entry,res", TABLE)
def test_entry_point_on_grid(entry, res):
    if entry == "normals":
        return _normals_case(res)
    # inputs first: every builder checks that queries stay within 8 cells of their targets
    facesp = _faces_pair(res)
    frozen = _frozen_pairs()
    decoy = _decoy_pair(res) if res in DECOY_SHIFTS else None
    for name, p in [("faces", facesp)] + [(n, q.moved(res - r0)) for n, (q, r0) in frozen.items()]:
        ka, kb = _keys(p.a, res), _keys(p.b, res)
        print(name, "res", res, len(p.a), len(p.b), "points; keys >= 2^31:", int((ka >= 2 ** 31).sum() + (kb >= 2 ** 31).sum()),
              ">= 2^32:", int((ka >= 2 ** 32).sum() + (kb >= 2 ** 32).sum()), "largest nearest d^2", p.near)
        assert (ka >= 2 ** 31).any() and (kb >= 2 ** 31).any() and max(ka.max(), kb.max()) < res ** 3
        assert res < 1626 or ((ka >= 2 ** 32).any() and (kb >= 2 ** 32).any())
    # the faces pair against brute force
    _agree(_run(entry, facesp, res), _faces_reference(res), "faces")
    for name, (p, r0) in frozen.items():
        home = _run(entry, p, r0)
        far = _run(entry, p.moved(res - r0), res)
        _same_bytes(far, home, name + " moved")
        if entry == "d2" and name in FROZEN_D2:
            assert [float(v).hex() for v in far["d2"]] == FROZEN_D2[name]
        if entry == "color_mse" and name == "faces_res64":
            assert [float(v).hex() for v in far["color_mse"]] == FROZEN_COLOR_MSE_FACES_RES64
        both = _run(entry, p.with_copy_at(res - r0, r0), res)
        _agree(both, _twice(home), name + " both ends")
        if entry == "d2":                                      # the maxima are order-free
            assert both["d2"][1] == home["d2"][1] and both["d2"][3] == home["d2"][3]
    if decoy is not None:
        _agree(_run(entry, decoy, res), _decoy_reference(res), "decoys")


# ---------------------------------------------------------------------------------------------------------------- second sweeps
@functools.lru_cache(maxsize=None)
def _sweep():
    """-> (Pair, A -> B, B -> A): a checkerboard of side 130 in the far corner of the 2048^3 grid, cloud A one parity (1 098 500
    points), cloud B the other with a seeded 30 % removed, so that distances (1, 3, 5, ...) and tie counts (1 .. 6 and more)
    vary; both in a seeded order.  The searches are the stencil's, which asserts d^2 <= 9 for every query of either side."""
    rng = np.random.default_rng(130)
    g = np.arange(SWEEP_SIDE)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    parity = cells.sum(1) % 2
    a, b = cells[parity == 0], cells[parity == 1]
    b = b[rng.random(len(b)) >= 0.3]
    a, b = (x[rng.permutation(len(x))] + (SWEEP_RES - SWEEP_SIDE) for x in (a, b))
    assert len(a) == 1098500 > 4096 * 256 and len(b) > 1024 * 256
    ab, ba = gref.tied(a, b), gref.tied(b, a)
    assert len(np.unique(ab.best)) >= 2 and len(np.unique(ab.count)) >= 6
    p = Pair(a.astype(np.int32), _colors_for(131, len(a)), _normals_for(132, len(a)), b.astype(np.int32), _colors_for(133, len(b)),
             near=int(max(ab.best.max(), ba.best.max())))
    return p, ab, ba


@functools.lru_cache(maxsize=None)
def _sweep_reference(entry):
    """what `entry` gives on the checkerboard, from the stencil's two searches"""
    p, ab, ba = _sweep()
    if entry == "d1":
        return {"d1": np.array(gref.d1(ab) + gref.d1(ba))}
    if entry == "d2":
        nb = gref.transfer_normals(ab, p.na)
        return {"normals_b": nb, "d2": np.array(gref.d2(ab, p.a, p.b, nb) + gref.d2(ba, p.b, p.a, p.na))}
    if entry == "recolor":
        colors, counts = gref.recolor(ab, ba, p.ca)
        return {"colors": colors, "counts": counts}
    return {"color_mse": np.r_[gref.color_mse(ab, p.ca, p.cb), gref.color_mse(ba, p.cb, p.ca)]}


@pytest.mark.parametrize("entry", sorted(RUN))
def test_second_sweep(entry):
    """more points than the largest launch covers in one sweep: 4.2 sweeps of the 1024-workgroup reductions (d1_partial_kernel,
    d2_partial_kernel, color_mse_partial_kernel), 1.05 of the 4096-workgroup scatters (recolor_scatter_kernel, d2_transfer_kernel)"""
    p, ref = _sweep()[0], _sweep_reference(entry)
    assert int(_keys(p.a, SWEEP_RES).min()) >= 2 ** 32
    got = _run(entry, p, SWEEP_RES)
    _agree(got, ref, "checkerboard")
    _same_bytes(_run(entry, p, SWEEP_RES), got, "a second run")


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_beyond_the_range_is_refused_and_touches_nothing():
    """res 4097 (resolution 4096 for the voxeliser) and, where the library refuses it (csrc/color.hip sizes_ok), n = 2^31: a
    non-zero return code, canary-filled outputs unchanged, and a sizing function that answers 0 where it validates.  At res 4096
    every workspace holds its bit sets: a size_t sum that wrapped would not."""
    lib, st, dev = _lib.hip(), _lib.stream(), _lib.require_gpu()
    P = _lib.dptr
    n = 4
    pts = _dev(np.int32([[0, 0, 0], [1, 2, 3], [4095, 4095, 4095], [7, 7, 7]]))
    col = _dev(_colors_for(1, n))
    nrm = _dev(_normals_for(1, n))
    keys = _dev(np.int64([0, 5, 9, 11]))
    fpts = pts.to(torch.float64)
    ws = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=dev)

    def canary(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(0xA5)
        return t
    out2, out3, nq = canary(4, torch.float64), canary(6, torch.float64), canary((n, 3), torch.float32)
    oc, on = canary((n, 3), torch.uint8), canary(n, torch.int32)
    vox, vcnt = canary((n, 3), torch.int32), canary(1, torch.int64)
    cov, knn = canary((n, 6), torch.int64), canary(n, torch.int32)
    outs = (out2, out3, nq, oc, on, vox, vcnt, cov, knn, ws)
    big = 2 ** 31
    calls = {
        "d1 res 4097": lambda: lib.pcgc_d1_mse(P(pts), n, P(pts), n, 4097, P(out2), P(ws), ws.numel(), st),
        "d2 transfer res 4097": lambda: lib.pcgc_d2_transfer_normals(P(pts), n, P(nrm), P(keys), n, 4097, P(nq), P(ws), ws.numel(), st),
        "d2 mse res 4097": lambda: lib.pcgc_d2_mse(P(pts), n, P(keys), n, P(nrm), 4097, P(out2), P(ws), ws.numel(), st),
        "recolor res 4097": lambda: lib.pcgc_recolor(P(pts), P(col), n, P(keys), n, 4097, P(oc), P(on), P(ws), ws.numel(), st),
        "recolor n_s 2^31": lambda: lib.pcgc_recolor(P(pts), P(col), big, P(keys), n, 64, P(oc), P(on), P(ws), ws.numel(), st),
        "recolor n_t 2^31": lambda: lib.pcgc_recolor(P(pts), P(col), n, P(keys), big, 64, P(oc), P(on), P(ws), ws.numel(), st),
        "color mse res 4097": lambda: lib.pcgc_color_mse(P(pts), P(col), n, P(pts), P(col), n, 4097, P(out3), P(ws), ws.numel(), st),
        "color mse n_a 2^31": lambda: lib.pcgc_color_mse(P(pts), P(col), big, P(pts), P(col), n, 64, P(out3), P(ws), ws.numel(), st),
        "color mse n_b 2^31": lambda: lib.pcgc_color_mse(P(pts), P(col), n, P(pts), P(col), big, 64, P(out3), P(ws), ws.numel(), st),
        "voxelize resolution 4096": lambda: lib.pcgc_mesh_voxelize(P(fpts), n, 4096, P(vox), n, P(vcnt), P(ws), ws.numel(), st),
        "normals res 4097": lambda: lib.pcgc_estimate_normals(P(pts), n, 4097, 10.0, 20, P(nq), P(cov), P(knn), P(ws), ws.numel(), st),
    }
    for what, call in calls.items():
        assert call() != 0, what
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.view(torch.uint8) == 0xA5).all())
    # the sizing functions that validate answer 0 (pcgc_d1_ and pcgc_d2_workspace_bytes do not validate)
    assert lib.pcgc_recolor_workspace_bytes(4097, n, n) == 0 and lib.pcgc_recolor_workspace_bytes(64, big, n) == 0
    assert lib.pcgc_recolor_workspace_bytes(64, n, big) == 0 and lib.pcgc_recolor_workspace_bytes(64, 0xFFFFFFFF // 255 + 1, n) == 0
    assert lib.pcgc_color_mse_workspace_bytes(4097, n) == 0 and lib.pcgc_color_mse_workspace_bytes(64, big) == 0
    assert lib.pcgc_mesh_voxelize_workspace_bytes(4096) == 0 and lib.pcgc_normals_workspace_bytes(4097, n, 10.0) == 0
    # the top of the range: res^3 / 8 bytes per bit set the workspace holds
    one = 4096 ** 3 // 8
    for entry, sets in BIT_SETS.items():
        got = _workspace_bytes(entry, 4096, 2500)
        print(entry, got, sets * one)
        assert sets * one <= got < sets * one + (1 << 26), (entry, got)
    got = int(lib.pcgc_mesh_voxelize_workspace_bytes(4095))
    assert one <= got < one + (1 << 26), got
