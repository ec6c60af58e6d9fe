"""D1 / D2 on the shared voxel grid (csrc/voxel_grid.h, csrc/tail.hip) against brute force in numpy: exact where the rule
is integer (D1, the transferred normals), to float64 rounding where it is a float sum (D2), and frozen to the bits the
kernels gave before the grid moved into one header — the order in which tied neighbours are visited is the order of D2's
and the colour mse's sums.  Workspace sizes are pinned to the same commit's."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _clouds import dense, faces                                         # noqa: E402
from pcgcv1_amd import _lib, metrics                                     # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _dist2(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return sum((a[:, None, k] - b[None, :, k]) ** 2 for k in range(3))


D1_CASES = {
    "faces_res64": (faces(10, 64, 1500)[0], faces(11, 64, 1200)[0]),
    "dense_res12": (dense(1, 12, 700)[0], dense(2, 12, 500)[0]),
    "one_each": (np.array([[3, 4, 5]], np.int32), np.array([[7, 1, 5]], np.int32)),
    "39_shells": (np.array([[0, 0, 0]], np.int32), np.array([[39, 39, 39]], np.int32)),
    "sparse_against_dense": (dense(5, 24, 60)[0], dense(6, 24, 2000)[0]),
}


@pytest.mark.parametrize("name", sorted(D1_CASES))
def test_d1_is_exact_against_brute_force(name):
    """Every term of D1 is an integer and the sums stay far below 2^53: the kernel's float64 sums are exact in any order and
    the division rounds once, so mse and the largest squared distance EQUAL numpy's, both directions."""
    a, b = D1_CASES[name]
    d = _dist2(a, b)
    m = metrics.d1_metrics(a, b, 1023)
    for way, near in (("1", d.min(1)), ("2", d.min(0))):
        want_mse, want_h = float(np.float64(int(near.sum())) / np.float64(len(near))), float(near.max())
        got_mse, got_h = m["mse%s      (p2point)" % way], m["h.       %s(p2point)" % way]
        print(name, way, got_mse, want_mse, got_h, want_h)
        assert got_mse == want_mse and got_h == want_h, (name, way, got_mse, want_mse, got_h, want_h)
    if name == "39_shells":
        assert m["h.        (p2point)"] == 3 * 39 * 39
    if name == "sparse_against_dense":
        assert m["h.        (p2point)"] == 74


def _d2_pair(seed, res, n_a, n_b):
    """two dense clouds in key order (the order pcgc_d2_* takes its target in) and seeded non-unit normals for the first"""
    a, b = dense(seed, res, n_a)[0], dense(seed + 1, res, n_b)[0]
    a, b = (p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))] for p in (a, b))
    rng = np.random.default_rng(100 + seed)
    na = (rng.normal(size=(len(a), 3)) * rng.uniform(0.5, 2.0, (len(a), 1))).astype(np.float32)
    return a, na, b, res


D2_CASES = {"dense_res12": _d2_pair(1, 12, 700, 500), "dense_res20": _d2_pair(3, 20, 1500, 2500)}

# float.hex() of (mse A->B, h. A->B, mse B->A, h. B->A) of _d2_device(*D2_CASES[name])[1], and of the six c[i] mse
# (A->B, then B->A) of the faces_res64 pair, from a build of the commit before csrc/voxel_grid.h on an MI355X
FROZEN_D2 = {
    "dense_res12": ["0x1.4fcd97efbb765p-1", "0x1.7ceee87120000p+3", "0x1.77eb92c06ef37p+0", "0x1.3704b13b819d0p+4"],
    "dense_res20": ["0x1.82fe25e2cf910p-1", "0x1.9c5f9efad4a40p+4", "0x1.c8dcbb161a734p+0", "0x1.426844e29e480p+5"],
}
FROZEN_COLOR_MSE_FACES_RES64 = ["0x1.947ddd4ec5b39p-4", "0x1.0920ae57ff2f1p-4", "0x1.45ae9a3b6dd17p-4",
                                "0x1.8cd3a742e772bp-4", "0x1.10ab4db0bba36p-4", "0x1.36ba45c866fe6p-4"]


def _d2_device(a, na, b, res):
    """pcgc_d2_transfer_normals A -> B, then pcgc_d2_mse both ways, as metrics.d2_metrics calls them
    -> (B's normals float32 [n_b, 3], the four float64 outputs)"""
    dev, lib = _lib.require_gpu(), _lib.hip()
    a_d, b_d, na_d = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (a, b, na))
    (ka, oa), (kb, ob) = metrics._sorted_keys(a_d, res), metrics._sorted_keys(b_d, res)
    assert bool((oa == torch.arange(len(a), device=dev)).all()) and bool((ob == torch.arange(len(b), device=dev)).all())
    ws = torch.empty(int(lib.pcgc_d2_workspace_bytes(res, max(len(a), len(b)))), dtype=torch.uint8, device=dev)
    nb_d = torch.empty((len(b), 3), dtype=torch.float32, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    st = _lib.stream()
    _lib.check(lib.pcgc_d2_transfer_normals(_lib.dptr(a_d), len(a), _lib.dptr(na_d), _lib.dptr(kb), len(b), res, _lib.dptr(nb_d),
                                            _lib.dptr(ws), ws.numel(), st), "pcgc_d2_transfer_normals")
    _lib.check(lib.pcgc_d2_mse(_lib.dptr(a_d), len(a), _lib.dptr(kb), len(b), _lib.dptr(nb_d), res, _lib.dptr(out), _lib.dptr(ws),
                               ws.numel(), st), "pcgc_d2_mse A->B")
    _lib.check(lib.pcgc_d2_mse(_lib.dptr(b_d), len(b), _lib.dptr(ka), len(a), _lib.dptr(na_d), res, _lib.dptr(out[2:]), _lib.dptr(ws),
                               ws.numel(), st), "pcgc_d2_mse B->A")
    return nb_d.cpu().numpy(), out.cpu().numpy()


def _plane(p, q, nq, tie):
    """per point of p: the mean over its tied nearest points of q of ((p - q) . normal(q))^2, in float64"""
    e = (p[:, None, :] - q[None, :, :]).astype(np.float64)
    n = nq.astype(np.float64)
    d = e[..., 0] * n[None, :, 0] + e[..., 1] * n[None, :, 1] + e[..., 2] * n[None, :, 2]
    return (d * d * tie).sum(1) / tie.sum(1)


@pytest.mark.parametrize("name", sorted(D2_CASES))
def test_d2_ties_against_brute_force(name):
    """Clouds dense enough that more than 30 % of the points of either side have two or more nearest targets.  The
    transferred normals follow an integer rule (llrint(n 2^40) summed in int64, float32(float64(sum) / 2^40 / count)) and
    EQUAL numpy's; the two mse and the two maxima are float64 sums, within 1e-12 relative of numpy's in another order (the
    margin test_color_metrics_against_pc_error_and_numpy uses); a second run gives the same bits; and the four float64
    equal, bit for bit, what the kernels gave before the shell search and the tie walk moved to csrc/voxel_grid.h:

        for name in sorted(D2_CASES): print(name, [float(v).hex() for v in _d2_device(*D2_CASES[name])[1]])"""
    a, na, b, res = D2_CASES[name]
    d = _dist2(a, b)
    tie_ab, tie_ba = d == d.min(1, keepdims=True), (d == d.min(0, keepdims=True)).T
    for tie in (tie_ab, tie_ba):
        share = float((tie.sum(1) >= 2).mean())
        print(name, "points with tied nearest targets: %.1f %%, up to %d" % (100 * share, tie.sum(1).max()))
        assert share > 0.30
    fixed = np.rint(na.astype(np.float64) * 2.0 ** 40).astype(np.int64)
    sums, count = tie_ab.T.astype(np.int64) @ fixed, tie_ab.sum(0)
    want_nb = np.where(count[:, None] > 0, sums.astype(np.float64) / 2.0 ** 40 / np.maximum(count, 1)[:, None], 0.0).astype(np.float32)
    got_nb, got = _d2_device(a, na, b, res)
    assert got_nb.tobytes() == want_nb.tobytes(), int((got_nb != want_nb).any(1).sum())
    p_ab, p_ba = _plane(a, b, want_nb, tie_ab), _plane(b, a, na, tie_ba)
    want = np.array([p_ab.mean(), p_ab.max(), p_ba.mean(), p_ba.max()])
    print(name, [float(v).hex() for v in got], want.tolist())
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    again_nb, again = _d2_device(a, na, b, res)
    assert again_nb.tobytes() == got_nb.tobytes() and again.tobytes() == got.tobytes()
    assert [float(v).hex() for v in got] == FROZEN_D2[name]


def test_color_mse_of_the_grid_faces_keeps_its_bits():
    """The six colour mse of the faces_res64 pair of test_gpu_color.py, with each cloud's own colours, equal bit for bit
    what the kernels gave before the grid moved to csrc/voxel_grid.h:

        m = metrics.color_metrics(*faces(10, 64, 1500), *faces(11, 64, 1200))
        print([m["c[%d],    %s" % (i, way)].hex() for way in "12" for i in range(3)])"""
    m = metrics.color_metrics(*faces(10, 64, 1500), *faces(11, 64, 1200))
    got = [m["c[%d],    %s" % (i, way)].hex() for way in "12" for i in range(3)]
    print(got)
    assert got == FROZEN_COLOR_MSE_FACES_RES64


# (res, n): pcgc_d1_, pcgc_d2_, pcgc_recolor_ (n_s = n_t = n), pcgc_color_mse_, pcgc_mesh_voxelize_ (resolution = res) and
# pcgc_normals_ (radius 10) _workspace_bytes of the commit before csrc/voxel_grid.h
WORKSPACE_BYTES = {
    (1, 1): (8452, 16692, 33792, 58112, 25088, 34816),
    (1, 2500): (8452, 86664, 83712, 68096, 25088, 214528),
    (12, 1): (8664, 16900, 33792, 58112, 25088, 34816),
    (12, 2500): (8664, 86872, 83712, 68096, 25088, 214528),
    (51, 1): (25032, 33268, 66560, 90880, 41472, 51200),
    (51, 2500): (25032, 103240, 116480, 100864, 41472, 230912),
    (64, 1): (41216, 49452, 66560, 90880, 57856, 51200),
    (64, 2500): (41216, 119424, 116480, 100864, 57856, 230912),
    (1024, 1): (134226176, 134234412, 268501760, 268526080, 134701568, 134301440),
    (1024, 2500): (134226176, 134304384, 268551680, 268536064, 134701568, 134481152),
}


def test_workspace_sizes_are_unchanged():
    """host arithmetic only: no kernel runs"""
    lib = _lib.hip()
    for (res, n), want in WORKSPACE_BYTES.items():
        got = (lib.pcgc_d1_workspace_bytes(res), lib.pcgc_d2_workspace_bytes(res, n), lib.pcgc_recolor_workspace_bytes(res, n, n),
               lib.pcgc_color_mse_workspace_bytes(res, n), lib.pcgc_mesh_voxelize_workspace_bytes(res),
               lib.pcgc_normals_workspace_bytes(res, n, 10.0))
        assert tuple(int(v) for v in got) == want, (res, n, got, want)
