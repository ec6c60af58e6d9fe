"""The simplification kernels (csrc/simplify.hip through pcgcv1_amd/surface.py: simplify) against the rule in numpy
(tests/_simplify_ref.py): vertices bit for bit, triangles equal as arrays (their order is part of the rule), every count of the
report equal.  The input is the reference's own mesh (tests/_surface_ref.py with given normals), so no normal estimation is in
the way; every mesh and every expected result is computed once per module."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _simplify_ref as sref                                             # noqa: E402
import _surface_ref as ref                                               # noqa: E402
from pcgcv1_amd import _lib, surface                                     # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402
from pcgcv1_amd.dataprocess import mesh2pc_open3d as m2p                 # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_sphere5_normals.npz")
C5 = (15.5, 15.5, 15.5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices, triangles, bits): the rule's mesh of a shape, its normals given"""
    if name in ("sphere", "rough"):
        # the golden normals come unoriented: propagated they give the closed sphere, taken as given a mesh full of folds, whose
        # simplification cancels triples and leaves clusters unused
        gold = np.load(GOLDEN)
        v, t, _ = ref.reconstruct(gold["points"], gold["normals"], 5, 3, mode="propagate" if name == "sphere" else "given")
        return v, t, 5
    elif name == "faces":                                                # touches 0 and res - 1 on every axis
        p, bits = ref.sphere(C5, 15.5), 5
        nr = ref.sphere_normals(p, C5)
    elif name == "torus":
        p, bits = ref.torus(), 5
        d = p - np.array(C5)
        rho = np.hypot(d[:, 0], d[:, 1])
        n = d - np.stack([d[:, 0] / rho * 9.0, d[:, 1] / rho * 9.0, 0 * rho], 1)
        nr = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    elif name == "patch":
        p, bits = ref.paraboloid(), 5
        n = np.stack([-(p[:, 0] - 15.5) / 12.0, -(p[:, 1] - 15.5) / 12.0, np.ones(len(p))], 1)
        nr = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    elif name == "two":
        ca, cb = (15.5, 15.5, 15.5), (45.5, 40.5, 40.5)
        a, b = ref.sphere(ca, 9.0), ref.sphere(cb, 11.0, seed=4)
        p, bits = np.r_[a, b], 6
        nr = np.r_[ref.sphere_normals(a, ca), ref.sphere_normals(b, cb)]
    else:
        raise KeyError(name)
    v, t, _ = ref.reconstruct(p, nr, bits, 3, mode="given")
    return v, t, bits


@functools.lru_cache(maxsize=None)
def rule(name, cell):
    v, t, bits = mesh(name)
    return sref.simplify(v, t, bits, cell)


def _same(got_v, got_t, report, want):
    want_v, want_t, want_report = want
    assert got_v.dtype == np.float64 and got_t.dtype == np.int32 and got_t.shape == want_t.shape and got_v.shape == want_v.shape
    differ = int((got_v != want_v).any(1).sum())
    assert got_v.tobytes() == want_v.tobytes(), "%d of %d vertices differ, at most by %g" % (differ, len(want_v), np.abs(got_v - want_v).max())
    np.testing.assert_array_equal(got_t, want_t)
    assert report == want_report


CASES = [("sphere", 1), ("sphere", 2), ("sphere", 3), ("sphere", 4), ("sphere", 16), ("faces", 5), ("torus", 2), ("torus", 8), ("patch", 2),
         ("two", 3), ("rough", 1), ("rough", 2)]


def test_the_meshes_are_what_the_cases_need():
    v, t, _ = mesh("sphere")
    assert (len(v), len(t)) == (6086, 12168)
    assert rule("sphere", 16)[2]["clusters"] == 8 and len(t) // 8 > 1000              # runs of more than a thousand triangles
    v, _, bits = mesh("faces")
    assert v.min() < 0 and v.max() > (1 << bits) - 1 and ((1 << bits) + 4) % 5 != 0    # M is a rounded-up quotient, the last cube partial
    assert len(mesh("two")[0]) > 10000 and mesh("two")[2] == 6
    _, _, count = sref.edge_balance(rule("torus", 8)[1])
    assert (count != 2).any()
    assert rule("rough", 1)[2]["cancelled"] > 0 and rule("rough", 1)[2]["unused"] > 0 and rule("rough", 2)[2]["merged"] > rule("rough", 2)[2]["cancelled"]


@pytest.mark.parametrize("name,cell", CASES)
def test_the_device_is_the_rule(name, cell):
    v, t, bits = mesh(name)
    want = rule(name, cell)
    report = {}
    got_v, got_t = surface.simplify(v, t, bits, cell, report=report)
    print("%s at cell %d: %s" % (name, cell, report))
    _same(got_v, got_t, report, want)
    assert tuple(report) == sref.REPORT_KEYS and report["folded"] == 0
    if name not in ("patch", "rough"):                                  # closed and consistently wound going in
        _, balance, _ = sref.edge_balance(got_t)
        assert (balance == 0).all()


def test_both_orders_of_the_triples_give_the_same_bytes():
    v, t, bits = mesh("sphere")
    for cell in (2, 16):
        for limit in (None, 1 << 21, 6086, 458, 457, 7, 0):             # the vertices and the clusters on either side of it
            report = {}
            got_v, got_t = surface.simplify(v, t, bits, cell, report=report, _pack_limit=limit)
            _same(got_v, got_t, report, rule("sphere", cell))
    # a cancelled, a folded and a merged triple through both
    one_v = np.array([[0.5, 0.5, 0.5], [5.5, 0.5, 0.25], [0.5, 7.5, 1.5], [0.75, 0.5, 0.5], [6.5, 6.5, 6.5]])
    tri = np.array([[0, 1, 2], [3, 1, 2], [0, 1, 4], [4, 1, 3], [2, 4, 1]], np.int32)
    want = sref.simplify(one_v, tri, 3, 2)
    assert want[2]["folded"] == 1 and want[2]["cancelled"] == 1 and want[2]["merged"] == 2
    for limit in (None, 0):
        report = {}
        got_v, got_t = surface.simplify(one_v, tri, 3, 2, report=report, _pack_limit=limit)
        _same(got_v, got_t, report, want)


def test_the_order_of_the_input_does_not_matter_and_two_calls_agree():
    v, t, bits = mesh("torus")
    rng = np.random.default_rng(3)
    perm, shift = rng.permutation(len(t)), rng.integers(0, 3, len(t))
    t2 = np.stack([t[perm, (shift + s) % 3] for s in range(3)], 1)
    for cell in (2, 8):
        a, b, c = surface.simplify(v, t, bits, cell), surface.simplify(v, t2, bits, cell), surface.simplify(v, t, bits, cell)
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
        _same(b[0], b[1], rule("torus", cell)[2], rule("torus", cell))


def test_tensors_in_tensors_out_and_the_empty_meshes():
    v, t, bits = mesh("sphere")
    dev = _lib.require_gpu()
    got_v, got_t = surface.simplify(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), bits, 3)
    assert torch.is_tensor(got_v) and got_v.is_cuda and got_t.dtype == torch.int32
    _same(got_v.cpu().numpy(), got_t.cpu().numpy(), rule("sphere", 3)[2], rule("sphere", 3))
    for tri, cell in ((t, 64), (np.zeros((0, 3), np.int32), 2), (t[:1], 1), (t[:1], 64)):
        report = {}
        got_v, got_t = surface.simplify(v, tri, bits, cell, report=report)
        _same(got_v, got_t, report, sref.simplify(v, tri, bits, cell))
    assert got_v.shape == (0, 3) and got_t.shape == (0, 3)
    report = {}
    got_v, got_t = surface.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.int32), 5, 2, report=report)
    assert got_v.shape == (0, 3) and got_t.shape == (0, 3) and report["clusters"] == 0


# ---------------------------------------------------------------------------- end to end
def test_reconstruct_simplifies_on_the_device():
    gold = np.load(GOLDEN)
    p, nr = gold["points"], gold["normals"]
    mv, mt, _ = mesh("sphere")
    plain_v, plain_t, plain = surface.reconstruct(p, nr, 5)              # without the option: what it returned before
    assert plain_v.tobytes() == mv.tobytes() and np.array_equal(surface.canonical(plain_t), ref.canonical(mt)) and "simplify" not in plain
    assert surface.summary_line(plain).count("\n") == 0
    v, t, report = surface.reconstruct(p, nr, 5, simplify=2)
    want = rule("sphere", 2)
    _same(v, t, report["simplify"], want)
    assert report["boundary_edges"] == 0 and (report["vertices"], report["triangles"]) == (len(want[0]), len(want[1]))
    assert {k: report[k] for k in ("voxels", "components", "rounds", "cells", "lattice_vertices")} == {
        k: plain[k] for k in ("voxels", "components", "rounds", "cells", "lattice_vertices")}
    assert surface.summary_line(report).splitlines()[1] == "simplify: cell 2, 6086 vertices and 12168 triangles -> %d and %d, %d of %d " \
        "clusters placed at their mean" % (len(want[0]), len(want[1]), want[2]["fallback"], want[2]["clusters"])
    from pcgcv1_amd import ingest
    frame = ingest.Frame((1.0, -2.0, 0.5), 0.25, 5)
    fv, ft, _ = surface.reconstruct(p, nr, None, frame=frame, simplify=2)            # simplified in voxel units, then the frame
    assert fv.tobytes() == ingest.apply_frame(want[0], frame).tobytes() and np.array_equal(ft, want[1])


def test_a_ply_through_the_command_line(tmp_path, monkeypatch, capsys):
    gold = np.load(GOLDEN)
    monkeypatch.chdir(tmp_path)
    iop.write_ply_normals("ball.ply", gold["points"], gold["normals"])
    surface.main(["--input", "ball.ply", "--output", "ball.obj", "--simplify", "2"])
    said = capsys.readouterr().out.splitlines()
    read_p, read_n = iop.load_ply_normals("ball.ply")                    # the normals as the ply's text holds them
    np.testing.assert_array_equal(read_p, gold["points"])
    mv, mt, _ = ref.reconstruct(read_p, read_n, 5, 3)
    want_v, want_t, want = sref.simplify(mv, mt, 5, 2)
    assert len(said) == 3 and said[0].startswith("surface: %d voxels, 1 components" % len(gold["points"])) and said[2] == "wrote ball.obj"
    assert said[0].endswith("%d vertices, %d triangles, 0 boundary edges" % (len(want_v), len(want_t)))
    assert said[1] == "simplify: cell 2, %d vertices and %d triangles -> %d and %d, %d of %d clusters placed at their mean" % (
        len(mv), len(mt), len(want_v), len(want_t), want["fallback"], want["clusters"])
    v, t = m2p.read_triangle_mesh("ball.obj")
    assert v.tobytes() == want_v.tobytes() and np.array_equal(t, want_t)


def test_decompress_hands_the_cell_to_the_mesh(tmp_path, monkeypatch, capsys):
    """--mesh_simplify reaches the mesh --mesh writes (the step decompress runs after the ply is on disk)"""
    import argparse
    from pcgcv1_amd import test as cli
    gold = np.load(GOLDEN)
    monkeypatch.chdir(tmp_path)
    iop.write_ply_data("ball_rec.ply", gold["points"])
    cli._mesh_output(argparse.Namespace(input="compressed/ball", output="ball_rec.ply", mesh="ball.obj", mesh_simplify=2))
    said = capsys.readouterr().out
    want_v, want_t, report = surface.reconstruct(iop.load_ply_data("ball_rec.ply"), simplify=2)
    assert surface.summary_line(report) in said and "\nsimplify: cell 2, " in said and "Mesh ball_rec.ply to ball.obj" in said
    v, t = m2p.read_triangle_mesh("ball.obj")
    assert v.tobytes() == want_v.tobytes() and np.array_equal(t, want_t) and 0 < len(t) < 2000


# ---------------------------------------------------------------------------- errors
def test_python_refuses_what_the_rule_excludes():
    v, t, bits = mesh("sphere")
    bad = v.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="vertex row 17.*not finite or lies outside"):
        surface.simplify(bad, t, bits, 2)
    bad = v.copy()
    bad[9, 2] = 34.0                                                     # res + 2
    with pytest.raises(ValueError, match="vertex row 9.*outside \\[-2, 34\\)"):
        surface.simplify(bad, t, bits, 2)
    bad[9, 2] = np.nextafter(34.0, 0.0)
    bad[5, 0] = np.nextafter(-2.0, -3.0)
    with pytest.raises(ValueError, match="vertex row 5"):
        surface.simplify(bad, t, bits, 2)
    bad_t = t.copy()
    bad_t[11, 2] = len(v)
    with pytest.raises(ValueError, match="triangle row 11.*outside 0..%d" % (len(v) - 1)):
        surface.simplify(v, bad_t, bits, 2)
    bad_t[11, 2] = -1
    with pytest.raises(ValueError, match="triangle row 11"):
        surface.simplify(v, bad_t, bits, 2)
    for cell in (0, 65):
        with pytest.raises(ValueError, match="cell = %d outside 1..64" % cell):
            surface.simplify(v, t, bits, cell)
        with pytest.raises(ValueError, match="cell = %d outside 1..64" % cell):
            surface.reconstruct(np.array([[1, 1, 1]], np.int32), np.array([[0, 0, 1]], np.float32), 3, simplify=cell)
    with pytest.raises(ValueError, match="bits"):
        surface.simplify(v, t, 13, 2)


def test_bad_arguments_touch_nothing_and_bad_rows_stay_in_bounds():
    lib, dev, s = _lib.hip(), _lib.require_gpu(), _lib.stream()
    v, t, bits = mesh("patch")
    V, T = len(v), len(t)
    vd, td = torch.from_numpy(v).to(dev), torch.from_numpy(surface.canonical(t).astype(np.int32)).to(dev)
    keys = torch.full((V,), -7, dtype=torch.int64, device=dev)
    for kw_bits, cell, n in ((bits, 0, V), (bits, 65, V), (0, 2, V), (13, 2, V), (bits, 2, 0)):
        assert lib.pcgc_simplify_keys(_lib.dptr(vd), n, kw_bits, cell, _lib.dptr(keys), s) == -1
        assert lib.pcgc_last_error().startswith(b"pcgc_simplify_keys")
    assert lib.pcgc_simplify_keys(None, V, bits, 2, _lib.dptr(keys), s) == -1
    rank = torch.zeros(V, dtype=torch.int32, device=dev)
    words = torch.full((T * 3,), -7, dtype=torch.int32, device=dev)
    sign = torch.full((T,), -7, dtype=torch.int32, device=dev)
    packed = torch.full((T,), -7, dtype=torch.int64, device=dev)
    assert lib.pcgc_simplify_incidence(_lib.dptr(td), T, _lib.dptr(rank), V, 0, _lib.dptr(words), s) == -1
    assert lib.pcgc_simplify_incidence(_lib.dptr(td), T, None, V, 1, _lib.dptr(words), s) == -1
    assert lib.pcgc_simplify_remap(_lib.dptr(td), T, _lib.dptr(rank), V, V + 1, _lib.dptr(words), _lib.dptr(sign), None, s) == -1
    big = (1 << 21) + 1
    assert lib.pcgc_simplify_remap(_lib.dptr(td), T, _lib.dptr(rank), big, big, _lib.dptr(words), _lib.dptr(sign), _lib.dptr(packed), s) == -1
    assert b"do not pack" in lib.pcgc_last_error()
    assert lib.pcgc_simplify_place(_lib.dptr(vd), V, _lib.dptr(td), T, _lib.dptr(keys), 1, bits, 2, None, None, None, None, None, None, s) == -1
    torch.cuda.synchronize()
    assert (keys == -7).all() and (words == -7).all() and (sign == -7).all() and (packed == -7).all()
    # rows the caller should have refused: the key kernel marks them, the triangle kernels treat their corners as no cluster
    bad = v.copy()
    bad[3, 0], bad[4, 1], bad[5, 2] = np.nan, 34.0, -2.5
    bd = torch.from_numpy(bad).to(dev)
    _lib.check(lib.pcgc_simplify_keys(_lib.dptr(bd), V, bits, 2, _lib.dptr(keys), s))
    good = torch.full((V,), -7, dtype=torch.int64, device=dev)
    _lib.check(lib.pcgc_simplify_keys(_lib.dptr(vd), V, bits, 2, _lib.dptr(good), s))
    assert keys[3:6].tolist() == [-1, -1, -1] and (keys[6:] == good[6:]).all() and (good >= 0).all()
    np.testing.assert_array_equal(torch.unique(good).cpu().numpy(), sref.clusters(v, bits, 2)[0])
    wild = td.clone()
    wild[0, 1], wild[1, 2] = V, -1
    _lib.check(lib.pcgc_simplify_incidence(_lib.dptr(wild), T, _lib.dptr(rank), V, 1, _lib.dptr(words), s))
    assert words[:6].tolist() == [0, 1, 1, 0, 1, 1] and (words.reshape(-1, 3)[2:] == torch.tensor([0, 1, 1], device=dev, dtype=torch.int32)).all()
    _lib.check(lib.pcgc_simplify_remap(_lib.dptr(wild), T, _lib.dptr(rank), V, 1, _lib.dptr(words), _lib.dptr(sign), _lib.dptr(packed), s))
    assert (words == -1).all() and (sign == 0).all() and (packed == -1).all()          # one cluster: every triangle is degenerate
