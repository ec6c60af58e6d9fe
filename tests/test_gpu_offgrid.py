"""D1 / D2 of clouds off the integer grid on the device (csrc/offgrid.hip, metrics.pc_error_float) against the rule in numpy
by brute force (tests/_offgrid_ref.py, pinned to the host path by test_offgrid_ref_host.py), against the host path and
against the answers of the prebuilt pc_error binary (tests/golden/pc_error_offgrid.npz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _offgrid_ref as ref                                               # noqa: E402
from _clouds import dense                                                # noqa: E402
from pcgcv1_amd import _lib, metrics                                     # noqa: E402

CASES = ref.cases()
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _reference(name):
    """the brute-force answer of a case, computed once and shared"""
    if name not in _REF:
        _REF[name] = ref.pc_error(*CASES[name], 1023)
    return _REF[name]


def _check_what_the_case_is_for(name, want):
    """on the reference's output, before the device is looked at: a change of inputs cannot quietly empty a case"""
    a, b, _ = CASES[name]
    ties1 = want["_1"]["n_ties"]
    if name == "s5_8":
        gap = np.abs(ref.dist2(a, want["_b"]) - want["_1"]["best"][:, None])
        tie = gap < ref.TIE
        assert (len(a), len(want["_b"])) == (1418, 786) and 0.03 < float((ties1 > 1).mean()) < 0.035
        assert 0 < gap[tie & (gap > 0)].max() < 1e-12 and 3e-7 < gap[~tie].min() < 4e-7
    elif name == "s3_4":
        gap = np.abs(ref.dist2(a, want["_b"]) - want["_1"]["best"][:, None])
        assert 7.9e-8 < gap[gap >= ref.TIE].min() < 8e-8
    elif name == "s8_5":
        assert np.unique(np.floor(want["_b"]), axis=0, return_counts=True)[1].max() == 4
    elif name == "far":                                       # 39 empty shells either way; direction 2 is the reverse
        assert want["_1"]["best"].tolist() == [39.5 ** 2 + 39.25 ** 2 + 39.75 ** 2] == want["_2"]["best"].tolist()
    elif name == "twelve_ties":                               # more than the 8 neighbours the host path asks its k-d tree for
        assert ties1.tolist() == [12] and want["_1"]["best"].tolist() == [4.5]
    elif name == "both_float":
        assert ties1.max() == 1 and want["_2"]["n_ties"].max() == 1 and metrics._off_grid(a) and metrics._off_grid(b)
    elif name == "rod_edge_2":
        assert a.min() < -700 and a[:, 0].max() - a[:, 0].min() > 1024 and metrics._off_grid(a)


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_point_outputs_and_figures_against_brute_force(name):
    """best, n_ties and the transferred normals EQUAL the reference's (float64 expressions in the stated association; an
    integer rule); plane[i] within 2 t_i 2^-53 relative (t_i non-negative terms in another order, then one division); each of
    the four figures within n 2^-52 relative of numpy's mean / max of the reference's per-point values, the maxima equal; a
    second run gives the same bytes.  Both directions."""
    a, b, na = CASES[name]
    want = _reference(name)
    _check_what_the_case_is_for(name, want)
    got, detail = metrics.pc_error_float(a, b, na, 1023, per_point=True)
    assert detail["normals_b"].tobytes() == want["_normals_b"].tobytes(), name
    for way in "12":
        w = want["_" + way]
        best, plane, ties = detail[way]
        n = len(best)
        assert best.tobytes() == w["best"].tobytes(), (name, way, int((best != w["best"]).sum()))
        assert np.array_equal(ties, w["n_ties"]), (name, way)
        err = np.abs(plane - w["plane"])
        print(name, way, "plane: largest error / bound %.3g" % float((err / np.maximum(2 * ties * 2.0 ** -53 * w["plane"], 1e-300)).max()))
        assert np.all(err <= 2 * ties * 2.0 ** -53 * w["plane"]), (name, way)
        for what, per_point in (("p2point", w["best"]), ("p2plane", w["plane"])):
            mse, h = got["mse%s      (%s)" % (way, what)], got["h.       %s(%s)" % (way, what)]
            print(name, way, what, mse, float(per_point.mean()), h, float(per_point.max()))
            assert abs(mse - per_point.mean()) <= n * 2.0 ** -52 * per_point.mean(), (name, way, what)
            assert h == per_point.max(), (name, way, what)
    again, detail2 = metrics.pc_error_float(a, b, na, 1023, per_point=True)
    assert again == got and detail2["normals_b"].tobytes() == detail["normals_b"].tobytes()
    for way in "12":
        assert all(x.tobytes() == y.tobytes() for x, y in zip(detail[way], detail2[way]))


GOLD = os.path.join(ROOT, "tests", "golden", "pc_error_offgrid.npz")


@pytest.mark.parametrize("i", range(3))
def test_golden_pairs_against_the_binary_and_the_host_path(i):
    """metrics.pc_error(..., off_grid="device") on the pairs the prebuilt pc_error measured: its printed values at the
    tolerances of test_metrics_offgrid.py; the host path's D1 keys within 1e-12 relative, its D2 keys within
    6 h max(1, max |normal|) 2^-41 absolute (h the host's h. (p2point)) plus 1e-12 relative — what rounding each normal
    component to 2^-40 fixed point can move ((p - q) . n)^2.  B reaches coordinate res and beyond."""
    g = np.load(GOLD)
    a, na, b, res = g["a%d" % i], g["na%d" % i], g["b%d" % i], int(g["res%d" % i])
    assert metrics._off_grid(b) and float(b.max()) >= res
    mine = metrics.pc_error(a, b, na, res - 1, off_grid="device")
    for k, want in zip([str(k) for k in g["keys"]], g["vals%d" % i]):
        tol = 1e-3 if "PSNR" in k else 2e-5 * max(1.0, abs(float(want)))
        print(i, k, mine[k], float(want))
        assert abs(mine[k] - float(want)) < tol, (i, k, mine[k], float(want))
    host = metrics.pc_error(a, b, na, res - 1)
    assert set(host) == set(mine)
    fixed = 6 * host["h.        (p2point)"] * max(1.0, float(np.abs(na).max())) * 2.0 ** -41
    for k, want in host.items():
        tol = 1e-12 * abs(want) + (fixed if "p2plane" in k else 0.0)
        print(i, k, mine[k], want, abs(mine[k] - want), tol)
        assert abs(mine[k] - want) <= tol, (i, k, mine[k], want, tol)


def test_integral_float_clouds_agree_with_the_grid_kernels():
    """every term is an integer there, so the sums are exact: the same dict as metrics.d1_metrics"""
    a, b = dense(21, 24, 900)[0], dense(22, 24, 700)[0]
    want = metrics.d1_metrics(a, b, 1023)
    got = metrics.pc_error_float(a.astype(np.float32), b.astype(np.float32), None, 1023)
    print(got, want)
    assert got == want


def test_the_cell_rule_refuses_what_it_cannot_hold():
    a = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match=r"2\^20"):           # extent / 1024 = 2^21
        metrics.pc_error_float(a, np.array([[0, 0, 0], [2.0 ** 31, 0, 0]], np.float32))
    with pytest.raises(ValueError, match="finite"):
        metrics.pc_error_float(a, np.array([[0, np.inf, 0]], np.float32))
    with pytest.raises(ValueError, match="float32"):
        metrics.pc_error_float(np.array([[0.1, 0, 0]], np.float64), a)


def test_a_target_that_breaks_the_contract_gives_nan_not_a_wrong_figure():
    """pcgc_offgrid_mse on a target that is not sorted by cell and has a point outside the stated grid: every index the
    kernels derive stays inside the workspace (include/pcgc.h), and the four figures come back as NaN"""
    dev, lib = _lib.require_gpu(), _lib.hip()
    q = torch.tensor([[5.5, 1, 1], [0.5, 1, 1], [9.5, 1, 1]], dtype=torch.float32, device=dev)          # descending, then outside
    p = torch.tensor([[0.25, 1, 1], [3, 3, 3]], dtype=torch.float32, device=dev)
    res = 8
    ws = torch.empty(int(lib.pcgc_offgrid_workspace_bytes(res, 3)), dtype=torch.uint8, device=dev)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    _lib.check(lib.pcgc_offgrid_mse(_lib.dptr(p), 2, _lib.dptr(q), 3, None, 1.0, 0, 0, 0, res, _lib.dptr(out), None, None, None,
                                    _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_offgrid_mse")
    assert bool(torch.isnan(out).all())
    assert lib.pcgc_offgrid_mse(_lib.dptr(p), 2, _lib.dptr(q), 3, None, 3.0, 0, 0, 0, res, _lib.dptr(out), None, None, None,
                                _lib.dptr(ws), ws.numel(), _lib.stream()) != 0            # an edge that is no power of two
    assert lib.pcgc_offgrid_workspace_bytes(1025, 3) == 0


def test_the_keyword_and_the_flag():
    a, b, _ = CASES["s5_8"]
    with pytest.raises(ValueError, match="off_grid"):
        metrics.pc_error(a, b, None, 1023, off_grid="bogus")
    with pytest.raises(ValueError, match="off_grid"):
        metrics.pc_error(a, a, None, 1023, off_grid="bogus")             # also for a cloud on the grid
    assert metrics.pc_error(a, b, None, 1023, off_grid="device") == metrics.pc_error_float(a, b, None, 1023)      # routed there
    r = subprocess.run([sys.executable, "-m", "pcgcv1_amd.eval", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--offgrid {host,device}" in r.stdout, r.stdout + r.stderr

